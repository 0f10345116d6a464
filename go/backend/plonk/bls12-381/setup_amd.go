//go:build amd

package plonk

/*
#include <stdlib.h>
#include "gnark_amd.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"unsafe"

	curve "github.com/consensys/gnark-crypto/ecc/bls12-381"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr/iop"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/kzg"
	"github.com/consensys/gnark/constraint"
	cs "github.com/consensys/gnark/constraint/bls12-381"
	"github.com/consensys/gnark/backend/plonk/internal"
)

// Setup is plonk.Setup (setup.go:108-171) on the GPU (gg_plonk_setup): the
// constraints go over as the arrays solver_amd.go builds (DecompressSparseR1C
// of every constraint instruction), the canonical SRS as it is; the Lagrange
// SRS (kzg.ToLagrangeG1, setup.go:134) is computed there by an EC-NTT.  The
// trace polynomials (canonical regular, setup.go:229-240), the permutation and
// the Lagrange SRS come back in gnark's memory layout and fill pk; the device
// key is built from the setup's results (gg_plonk_setup_pk) and registered for
// pk, so the first Prove finds it; the vk digests are that key's commitTrace
// (gg_plonk_pk_vk).  gnark's CPU Setup is setupCPU (setup_noamd.go).
func Setup(spr *cs.SparseR1CS, kzgSrs kzg.SRS) (*ProvingKey, *VerifyingKey, error) {
	var pk ProvingKey
	var vk VerifyingKey
	pk.Vk = &vk
	vk.CommitmentConstraintIndexes = internal.IntSliceToUint64Slice(spr.CommitmentInfo.CommitmentIndexes())

	pk.initDomains(spr)
	if pk.Domain[0].Cardinality < 2 {
		return nil, nil, fmt.Errorf("circuit has only %d constraints; unsupported by the current implementation", spr.GetNbConstraints())
	}
	pk.Vk.CosetShift.Set(&pk.Domain[0].FrMultiplicativeGen)
	vk.Size = pk.Domain[0].Cardinality
	vk.SizeInv.SetUint64(vk.Size).Inverse(&vk.SizeInv)
	vk.Generator.Set(&pk.Domain[0].Generator)
	vk.NbPublicVariables = uint64(len(spr.Public))
	n := int(vk.Size)
	if len(kzgSrs.Pk.G1) < n+3 {
		return nil, nil, errors.New("kzg srs is too small")
	}
	pk.Kzg.G1 = kzgSrs.Pk.G1[:n+3]
	vk.Kzg = kzgSrs.Vk

	nbCons := spr.GetNbConstraints()
	wires := make([]uint32, 0, 3*nbCons)
	qidx := make([]uint32, 0, 5*nbCons)
	it := spr.GetSparseR1CIterator()
	for c := it.Next(); c != nil; c = it.Next() {
		wires = append(wires, c.XA, c.XB, c.XC)
		qidx = append(qidx, c.QL, c.QR, c.QO, c.QM, c.QC)
	}
	commitmentInfo := spr.CommitmentInfo.(constraint.PlonkCommitments)
	committedOff := make([]uint32, 1, len(commitmentInfo)+1)
	var committed []uint32
	for i := range commitmentInfo {
		for _, k := range commitmentInfo[i].Committed {
			committed = append(committed, uint32(k))
		}
		committedOff = append(committedOff, uint32(len(committed)))
	}
	cmtIdx := append(append([]uint64{}, vk.CommitmentConstraintIndexes...), 0)
	nbVariables := spr.NbInternalVariables + len(spr.Public) + len(spr.Secret)
	if len(spr.Coefficients) == 0 {
		return nil, nil, errors.New("gnark_amd: empty coefficient table")
	}

	devs := amdConfiguredDevices()
	cdevs := make([]C.int, len(devs)+1)
	for i, d := range devs {
		cdevs[i] = C.int(d)
	}
	nPoly := 8 + len(commitmentInfo)
	polys := make([][]fr.Element, nPoly)
	pk.trace.S = make([]int64, 3*n)
	pk.KzgLagrange.G1 = make([]curve.G1Affine, n)
	digests := make([]curve.G1Affine, nPoly)
	var key C.gg_plonk_pk_t
	if err := onAMDDevice(amdPrimaryDevice(), func() error {
		var h C.gg_plonk_setup_t
		if C.gg_plonk_setup(amdCurve, C.size_t(nbVariables), C.size_t(nbCons), C.size_t(len(spr.Public)),
			u32p(wires), u32p(qidx), unsafe.Pointer(&spr.Coefficients[0]), C.size_t(len(spr.Coefficients)),
			C.int(len(commitmentInfo)), u32p(committedOff), u32p(committed),
			(*C.uint64_t)(unsafe.Pointer(&cmtIdx[0])), unsafe.Pointer(&pk.Domain[0].Generator),
			unsafe.Pointer(&pk.Domain[0].FrMultiplicativeGen), unsafe.Pointer(&pk.Kzg.G1[0]),
			C.size_t(len(pk.Kzg.G1)), nil, &h) != C.GG_OK {
			return amdError()
		}
		defer C.gg_plonk_setup_release(h)
		for i := range polys {
			polys[i] = make([]fr.Element, n)
			which := C.GG_PLONK_SETUP_QL + i
			if i >= 8 {
				which = C.GG_PLONK_SETUP_QCP + i - 8
			}
			if C.gg_plonk_setup_read(h, C.int(which), unsafe.Pointer(&polys[i][0]), C.size_t(n*fr.Bytes)) != C.GG_OK {
				return amdError()
			}
		}
		if C.gg_plonk_setup_read(h, C.GG_PLONK_SETUP_PERM, unsafe.Pointer(&pk.trace.S[0]), C.size_t(3*n*8)) != C.GG_OK {
			return amdError()
		}
		if C.gg_plonk_setup_read(h, C.GG_PLONK_SETUP_LAGRANGE, unsafe.Pointer(&pk.KzgLagrange.G1[0]),
			C.size_t(uintptr(n)*unsafe.Sizeof(pk.KzgLagrange.G1[0]))) != C.GG_OK {
			return amdError()
		}
		if C.gg_plonk_setup_pk(h, unsafe.Pointer(&pk.Domain[1].Generator), C.int(len(devs)), &cdevs[0], &key) != C.GG_OK {
			return amdError()
		}
		if C.gg_plonk_pk_vk(key, unsafe.Pointer(&digests[0]), C.size_t(uintptr(nPoly)*unsafe.Sizeof(digests[0]))) != C.GG_OK {
			C.gg_plonk_pk_release(key)
			return amdError()
		}
		return nil
	}); err != nil {
		return nil, nil, err
	}
	canReg := iop.Form{Basis: iop.Canonical, Layout: iop.Regular}
	tr := []**iop.Polynomial{&pk.trace.Ql, &pk.trace.Qr, &pk.trace.Qm, &pk.trace.Qo, &pk.trace.Qk,
		&pk.trace.S1, &pk.trace.S2, &pk.trace.S3}
	for i, p := range tr {
		*p = iop.NewPolynomial(&polys[i], canReg)
	}
	pk.trace.Qcp = make([]*iop.Polynomial, len(commitmentInfo))
	for i := range pk.trace.Qcp {
		pk.trace.Qcp[i] = iop.NewPolynomial(&polys[8+i], canReg)
	}
	// gg_plonk_pk_vk: S1, S2, S3, Ql, Qr, Qm, Qo, Qk, Qcp...
	copy(vk.S[:], digests[0:3])
	vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk = digests[3], digests[4], digests[5], digests[6], digests[7]
	vk.Qcp = append([]curve.G1Affine{}, digests[8:]...)
	amdKeys.Store(&pk, key)
	return &pk, &vk, nil
}

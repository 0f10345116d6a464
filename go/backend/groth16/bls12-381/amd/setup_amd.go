//go:build amd

package amd_bls12381

/*
#include <stdlib.h>
#include "gnark_amd.h"
*/
import "C"

import (
	"bytes"
	"fmt"
	"unsafe"

	curve "github.com/consensys/gnark-crypto/ecc/bls12-381"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr/fft"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr/pedersen"
	groth16_bls12381 "github.com/consensys/gnark/backend/groth16/bls12-381"
	"github.com/consensys/gnark/constraint"
	cs "github.com/consensys/gnark/constraint/bls12-381"
)

// sampleNonZero is one draw of sampleToxicWaste (setup.go:444-478).
func sampleNonZero() (fr.Element, error) {
	var e fr.Element
	for e.IsZero() {
		if _, err := e.SetRandom(); err != nil {
			return e, err
		}
	}
	return e, nil
}

// Setup is groth16.Setup (backend/groth16/bls12-381/setup.go:85-337) on the GPU
// (gg_groth16_setup): the R1Cs go over as the CSR solver_amd.go builds, the
// toxic waste is sampled here as sampleToxicWaste does, the key's points come
// back in gnark's memory layout and fill pk and vk; vk.Precompute() (the
// pairing e) runs on the host.  Setup needs only the matrices, so a system
// whose hints keep gnark's solver is set up here all the same.
func Setup(r1cs *cs.R1CS, pk *ProvingKey, vk *groth16_bls12381.VerifyingKey) error {
	rs := r1cs.GetR1Cs()
	off := make([]uint32, 1, 3*len(rs)+1)
	var wires, coeffs []uint32
	for _, c := range rs {
		for _, le := range []constraint.LinearExpression{c.L, c.R, c.O} {
			for _, t := range le {
				w := uint32(t.WireID())
				if t.IsConstant() { // coeff * ONE_WIRE (term.go:35-41)
					w = 0
				}
				wires = append(wires, w)
				coeffs = append(coeffs, uint32(t.CoeffID()))
			}
			off = append(off, uint32(len(wires)))
		}
	}
	nbPublic := r1cs.GetNbPublicVariables()
	nbWires := nbPublic + r1cs.GetNbSecretVariables() + r1cs.NbInternalVariables
	if len(rs) == 0 || len(r1cs.Coefficients) == 0 {
		return fmt.Errorf("gnark_amd: empty constraint system")
	}

	commitmentInfo := r1cs.CommitmentInfo.(constraint.Groth16Commitments)
	commitmentWires := commitmentInfo.CommitmentIndexes()
	privateCommitted := commitmentInfo.GetPrivateCommitted()
	cw := make([]uint32, len(commitmentWires))
	for i, w := range commitmentWires {
		cw[i] = uint32(w)
	}
	committedOff := make([]uint32, 1, len(privateCommitted)+1)
	var committed []uint32
	for _, pc := range privateCommitted {
		for _, w := range pc {
			committed = append(committed, uint32(w))
		}
		committedOff = append(committedOff, uint32(len(committed)))
	}

	// toxic waste (setup.go:113-117) and pedersen.Setup's sigma and G = g * G2
	var tw [7]fr.Element // tau, alpha, beta, gamma, delta, sigma, g
	for i := range tw {
		e, err := sampleNonZero()
		if err != nil {
			return err
		}
		tw[i] = e
	}
	domain := fft.NewDomain(uint64(len(rs)))
	_, _, g1, g2 := curve.Generators()

	var h C.gg_g16_setup_t
	if C.gg_groth16_setup(C.GG_CURVE_BLS12_381, C.size_t(nbWires), C.size_t(len(rs)), C.size_t(nbPublic),
		u32p(off), u32p(wires), u32p(coeffs), unsafe.Pointer(&r1cs.Coefficients[0]),
		C.size_t(len(r1cs.Coefficients)), u32p(cw), C.size_t(len(cw)), u32p(committedOff), u32p(committed),
		unsafe.Pointer(&tw[0]), unsafe.Pointer(&tw[1]), unsafe.Pointer(&tw[2]), unsafe.Pointer(&tw[3]),
		unsafe.Pointer(&tw[4]), unsafe.Pointer(&tw[5]), unsafe.Pointer(&tw[6]),
		unsafe.Pointer(&domain.Generator), unsafe.Pointer(&g1), unsafe.Pointer(&g2), &h) != C.GG_OK {
		return lastError()
	}
	defer C.gg_groth16_setup_release(h)
	for i := range tw { // the host copies of the toxic waste
		tw[i].SetZero()
	}

	var logN C.int
	var nA, nB, nK, nZ, nVkK, nCom, chunk, launches C.size_t
	nCk := make([]C.size_t, len(cw)+1)
	if C.gg_groth16_setup_info(h, &logN, &nA, &nB, &nK, &nZ, &nVkK, &nCom, &nCk[0], C.size_t(len(cw)),
		&chunk, &launches) != C.GG_OK {
		return lastError()
	}
	g1s := func(which int, n C.size_t) ([]curve.G1Affine, error) {
		out := make([]curve.G1Affine, int(n))
		if n == 0 {
			return out, nil
		}
		if C.gg_groth16_setup_read(h, C.int(which), unsafe.Pointer(&out[0]),
			C.size_t(uintptr(n)*unsafe.Sizeof(out[0]))) != C.GG_OK {
			return nil, lastError()
		}
		return out, nil
	}
	g2s := func(which int, n C.size_t) ([]curve.G2Affine, error) {
		out := make([]curve.G2Affine, int(n))
		if n == 0 {
			return out, nil
		}
		if C.gg_groth16_setup_read(h, C.int(which), unsafe.Pointer(&out[0]),
			C.size_t(uintptr(n)*unsafe.Sizeof(out[0]))) != C.GG_OK {
			return nil, lastError()
		}
		return out, nil
	}
	flags := func(which int) ([]bool, uint64, error) {
		raw := make([]byte, nbWires)
		if C.gg_groth16_setup_read(h, C.int(which), unsafe.Pointer(&raw[0]), C.size_t(nbWires)) != C.GG_OK {
			return nil, 0, lastError()
		}
		out := make([]bool, nbWires)
		var nb uint64
		for i, b := range raw {
			if b != 0 {
				out[i] = true
				nb++
			}
		}
		return out, nb, nil
	}

	var err error
	if pk.G1.A, err = g1s(C.GG_SETUP_G1_A, nA); err != nil {
		return err
	}
	if pk.G1.B, err = g1s(C.GG_SETUP_G1_B, nB); err != nil {
		return err
	}
	if pk.G1.K, err = g1s(C.GG_SETUP_G1_K, nK); err != nil {
		return err
	}
	if pk.G1.Z, err = g1s(C.GG_SETUP_G1_Z, nZ); err != nil {
		return err
	}
	if pk.G2.B, err = g2s(C.GG_SETUP_G2_B, nB); err != nil {
		return err
	}
	if vk.G1.K, err = g1s(C.GG_SETUP_VK_K, nVkK); err != nil {
		return err
	}
	one1 := func(which int, dst *curve.G1Affine) error {
		p, e := g1s(which, 1)
		if e == nil {
			*dst = p[0]
		}
		return e
	}
	one2 := func(which int, dst *curve.G2Affine) error {
		p, e := g2s(which, 1)
		if e == nil {
			*dst = p[0]
		}
		return e
	}
	for _, e := range []error{
		one1(C.GG_SETUP_ALPHA1, &pk.G1.Alpha), one1(C.GG_SETUP_BETA1, &pk.G1.Beta),
		one1(C.GG_SETUP_DELTA1, &pk.G1.Delta), one2(C.GG_SETUP_BETA2, &pk.G2.Beta),
		one2(C.GG_SETUP_DELTA2, &pk.G2.Delta), one2(C.GG_SETUP_GAMMA2, &vk.G2.Gamma),
	} {
		if e != nil {
			return e
		}
	}
	if pk.InfinityA, pk.NbInfinityA, err = flags(C.GG_SETUP_INFINITY_A); err != nil {
		return err
	}
	if pk.InfinityB, pk.NbInfinityB, err = flags(C.GG_SETUP_INFINITY_B); err != nil {
		return err
	}

	// commitment keys (setup.go:280-295).  pedersen.ProvingKey keeps its bases
	// unexported in the pinned gnark-crypto, so each key goes through its own
	// ReadFrom (the encoding WriteTo produces: basis, then basisExpSigma).
	pk.CommitmentKeys = make([]pedersen.ProvingKey, int(nCom))
	for j := range pk.CommitmentKeys {
		basis, e := g1s(C.GG_SETUP_CK_BASIS+j, nCk[j])
		if e != nil {
			return e
		}
		basisExpSigma, e := g1s(C.GG_SETUP_CK_BASIS_SIGMA+j, nCk[j])
		if e != nil {
			return e
		}
		var buf bytes.Buffer
		enc := curve.NewEncoder(&buf, curve.RawEncoding())
		if e = enc.Encode(basis); e != nil {
			return e
		}
		if e = enc.Encode(basisExpSigma); e != nil {
			return e
		}
		if _, e = pk.CommitmentKeys[j].ReadFrom(&buf); e != nil {
			return e
		}
	}
	if nCom > 0 {
		pv, e := g2s(C.GG_SETUP_PEDERSEN_VK, 2)
		if e != nil {
			return e
		}
		vk.CommitmentKey.G, vk.CommitmentKey.GRootSigmaNeg = pv[0], pv[1]
	}
	vk.PublicAndCommitmentCommitted = commitmentInfo.GetPublicAndCommitmentCommitted(commitmentWires, nbPublic)

	// setup.go:320-334
	vk.G1.Alpha, vk.G1.Beta, vk.G1.Delta = pk.G1.Alpha, pk.G1.Beta, pk.G1.Delta
	vk.G2.Beta, vk.G2.Delta = pk.G2.Beta, pk.G2.Delta
	if err := vk.Precompute(); err != nil {
		return err
	}
	pk.Domain = *domain
	return nil
}

//go:build amd

package amd_bls12381

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
	groth16_bls12381 "github.com/consensys/gnark/backend/groth16/bls12-381"
)

// the errors of groth16.Verify (backend/groth16/bls12-381/verify.go:35-38)
var (
	errPairingCheckFailed         = errors.New("pairing doesn't match")
	errCorrectSubgroupCheckFailed = errors.New("points in the proof are not in the correct subgroup")
	errCommitmentPok              = errors.New("failed to verify the commitments' proof of knowledge")
)

// VerifyingKey is a groth16 VerifyingKey prepared for batches of proofs
// (gg_groth16_vk_create_bls12_381): -gamma, -delta, the line tables of the fixed
// G2 operands and e(alpha, beta), computed on the host.  The first VerifyBatch
// uploads the key and builds the window table of K[1:]; VerifyBatchHost needs
// no GPU.
type VerifyingKey struct {
	nbPublic      int
	nbCommitments int
	released      bool
	handle        interface{}
}

// NewVerifyingKey prepares vk.  The Pedersen key's two points are passed
// explicitly because gnark keeps them in unexported fields; K and
// PublicAndCommitmentCommitted are vk's own.
func NewVerifyingKey(vk *groth16_bls12381.VerifyingKey, pedersenG, pedersenGRootSigmaNeg *curve.G2Affine) (*VerifyingKey, error) {
	nc := len(vk.PublicAndCommitmentCommitted)
	off := make([]uint32, 1, nc+1)
	var idx []uint32
	for _, c := range vk.PublicAndCommitmentCommitted {
		for _, i := range c {
			idx = append(idx, uint32(i))
		}
		off = append(off, uint32(len(idx)))
	}
	var pg, pgs unsafe.Pointer
	var offp, idxp *C.uint32_t
	if nc > 0 {
		if pedersenG == nil || pedersenGRootSigmaNeg == nil {
			return nil, fmt.Errorf("gnark_amd: the key has commitments: the Pedersen verifying key is needed")
		}
		pg, pgs = unsafe.Pointer(pedersenG), unsafe.Pointer(pedersenGRootSigmaNeg)
		offp = u32p(off)
		idxp = u32p(idx)
	}
	var h C.gg_groth16_vk_bls_t
	if C.gg_groth16_vk_create_bls12_381(unsafe.Pointer(&vk.G1.Alpha), unsafe.Pointer(&vk.G2.Beta),
		unsafe.Pointer(&vk.G2.Gamma), unsafe.Pointer(&vk.G2.Delta), unsafe.Pointer(&vk.G1.K[0]),
		C.size_t(len(vk.G1.K)), C.size_t(len(vk.G1.K)-nc), pg, pgs, offp, idxp, C.int(nc), &h) != C.GG_OK {
		return nil, lastError()
	}
	return &VerifyingKey{nbPublic: len(vk.G1.K) - nc, nbCommitments: nc, handle: h}, nil
}

// Release frees the key.
func (d *VerifyingKey) Release() {
	if !d.released {
		C.gg_groth16_vk_destroy_bls12_381(d.handle.(C.gg_groth16_vk_bls_t))
		d.released = true
	}
}

// VerifyBatch is groth16.Verify (verify.go:42-140) for every proof under one
// key on the GPU: errs[i] is nil, errCorrectSubgroupCheckFailed, the Pedersen
// error or errPairingCheckFailed, decided per proof (no random linear combination).
func (d *VerifyingKey) VerifyBatch(proofs []*groth16_bls12381.Proof, witnesses []fr.Vector) ([]error, error) {
	return d.verifyBatch(proofs, witnesses, false)
}

// VerifyBatchHost runs the same per-proof functions on the calling thread.
func (d *VerifyingKey) VerifyBatchHost(proofs []*groth16_bls12381.Proof, witnesses []fr.Vector) ([]error, error) {
	return d.verifyBatch(proofs, witnesses, true)
}

func (d *VerifyingKey) verifyBatch(proofs []*groth16_bls12381.Proof, witnesses []fr.Vector, host bool) ([]error, error) {
	n := len(proofs)
	if n == 0 || n != len(witnesses) {
		return nil, fmt.Errorf("gnark_amd: %d proofs, %d witnesses", n, len(witnesses))
	}
	nw := d.nbPublic - 1
	type packed struct {
		Ar  curve.G1Affine
		Bs  curve.G2Affine
		Krs curve.G1Affine
	}
	pp := make([]packed, n)
	cm := make([]curve.G1Affine, n*d.nbCommitments+1)
	pok := make([]curve.G1Affine, n)
	wit := make([]fr.Element, n*nw+1)
	for i, p := range proofs {
		if len(witnesses[i]) != nw {
			return nil, fmt.Errorf("invalid witness size, got %d, expected %d (public - ONE_WIRE)", len(witnesses[i]), nw)
		}
		if len(p.Commitments) != d.nbCommitments {
			return nil, fmt.Errorf("gnark_amd: proof %d has %d commitments, the key %d", i, len(p.Commitments), d.nbCommitments)
		}
		pp[i] = packed{p.Ar, p.Bs, p.Krs}
		copy(cm[i*d.nbCommitments:], p.Commitments)
		pok[i] = p.CommitmentPok
		copy(wit[i*nw:], witnesses[i])
	}
	var cmp, pokp, witp unsafe.Pointer
	if d.nbCommitments > 0 {
		cmp, pokp = unsafe.Pointer(&cm[0]), unsafe.Pointer(&pok[0])
	}
	if nw > 0 {
		witp = unsafe.Pointer(&wit[0])
	}
	status := make([]uint8, n)
	var rc C.int
	if host {
		rc = C.gg_groth16_verify_batch_bls12_381_host(d.handle.(C.gg_groth16_vk_bls_t), C.size_t(n), unsafe.Pointer(&pp[0]),
			cmp, pokp, witp, (*C.uint8_t)(unsafe.Pointer(&status[0])))
	} else {
		rc = C.gg_groth16_verify_batch_bls12_381(d.handle.(C.gg_groth16_vk_bls_t), C.size_t(n), unsafe.Pointer(&pp[0]),
			cmp, pokp, witp, (*C.uint8_t)(unsafe.Pointer(&status[0])))
	}
	if rc != C.GG_OK {
		return nil, lastError()
	}
	errs := make([]error, n)
	for i, s := range status {
		switch s {
		case C.GG_VERIFY_OK:
		case C.GG_VERIFY_SUBGROUP:
			errs[i] = errCorrectSubgroupCheckFailed
		case C.GG_VERIFY_PEDERSEN:
			errs[i] = errCommitmentPok
		default:
			errs[i] = errPairingCheckFailed
		}
	}
	return errs, nil
}

// Verify is groth16.Verify for one proof.
func (d *VerifyingKey) Verify(proof *groth16_bls12381.Proof, publicWitness fr.Vector) error {
	errs, err := d.VerifyBatch([]*groth16_bls12381.Proof{proof}, []fr.Vector{publicWitness})
	if err != nil {
		return err
	}
	return errs[0]
}

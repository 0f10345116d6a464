//go:build !amd

package plonk

import (
	"github.com/consensys/gnark-crypto/ecc/bls12-381/kzg"
	cs "github.com/consensys/gnark/constraint/bls12-381"
)

// Setup without the build tag is gnark's CPU Setup (setup.go:108-171, kept in
// setup.go as setupCPU).
func Setup(spr *cs.SparseR1CS, kzgSrs kzg.SRS) (*ProvingKey, *VerifyingKey, error) {
	return setupCPU(spr, kzgSrs)
}

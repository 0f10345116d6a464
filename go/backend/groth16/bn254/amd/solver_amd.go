//go:build amd

package amd_bn254

/*
#include <stdlib.h>
#include "gnark_amd.h"
*/
import "C"

import (
	"fmt"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark/backend/witness"
	"github.com/consensys/gnark/constraint"
	cs "github.com/consensys/gnark/constraint/bn254"
)

// deviceSolver is r1cs.Solve on the GPU (constraint/bn254/solver.go:418-608)
// for systems whose hint calls are all gnark's built-in ones (gg_hint_supported;
// none at all included): the R1Cs, the hint instructions, the coefficient table
// and the levels are uploaded once (gg_r1cs_create), and a solve leaves W, A, B, C in
// HBM for gg_groth16_prove (inputs_on_device = 1) -- only the witness crosses
// PCIe.  Built lazily next to setupDevicePointers; nil for systems with any
// other hint (user-defined, BSB22 commitment, emulated arithmetic, lookup,
// selector: hints are Go functions, those keep gnark's solver).  The caller
// asks for a device solver only when the prover got no solver options, so no
// option can override or add a function for one of the system's hint ids.  A multi-GPU key has one
// solver per device, each leaving the whole solution on its GPU
// (gg_groth16_mpk_prove_ex reads shard r's copy on devices[r]).
type deviceSolver struct {
	h        C.gg_r1cs_t
	nbWires  int
	nbCons   int
	nbInputs int // witness length: nbPublic - 1 + nbSecret (solver.go:71-76)
}

// hintArrays is the system's hint instructions in the layout of
// gg_r1cs_set_hints (BlueprintGenericHint.DecompressHint of each).
type hintArrays struct {
	ids, inOff, exprOff, wires, coeffs, outStart, outEnd []uint32
}

func (ha *hintArrays) add(hm *constraint.HintMapping) {
	ha.ids = append(ha.ids, uint32(hm.HintID))
	for _, le := range hm.Inputs {
		for _, t := range le {
			w := uint32(t.WireID())
			if t.IsConstant() { // coeff * ONE_WIRE (term.go:35-41)
				w = 0
			}
			ha.wires = append(ha.wires, w)
			ha.coeffs = append(ha.coeffs, uint32(t.CoeffID()))
		}
		ha.exprOff = append(ha.exprOff, uint32(len(ha.wires)))
	}
	ha.inOff = append(ha.inOff, uint32(len(ha.exprOff)-1))
	ha.outStart = append(ha.outStart, hm.OutputRange.Start)
	ha.outEnd = append(ha.outEnd, hm.OutputRange.End)
}

// u32p is &s[0], or nil for an empty slice.
func u32p(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}

// newDeviceSolvers builds the CSR form of the system once and uploads it to
// every distinct device of devs (nil map: the system has a hint the library
// does not evaluate, or an instruction that is neither an R1C nor a hint).
func newDeviceSolvers(sys *cs.R1CS, devs []int) (map[int]*deviceSolver, error) {
	// instruction ids are not constraint ids once hints are in: an R1C
	// instruction maps to its constraint index, a hint instruction to its
	// hint index (r1cs.Levels holds instruction ids)
	const isHint = uint32(1) << 31
	instTo := make([]uint32, len(sys.Instructions))
	ha := hintArrays{inOff: []uint32{0}, exprOff: []uint32{0}}
	var hm constraint.HintMapping
	for i, pi := range sys.Instructions {
		switch bp := sys.Blueprints[pi.BlueprintID].(type) {
		case constraint.BlueprintHint:
			bp.DecompressHint(&hm, pi.Unpack(&sys.System))
			var ok C.int
			if C.gg_hint_supported(C.uint32_t(hm.HintID), &ok, nil) != C.GG_OK || ok == 0 {
				return nil, nil // not one of gnark's built-in hints: gnark's solver
			}
			instTo[i] = isHint | uint32(len(ha.ids))
			ha.add(&hm)
		case constraint.BlueprintR1C:
			instTo[i] = pi.ConstraintOffset // one R1C per instruction
		default:
			return nil, nil
		}
	}
	rs := sys.GetR1Cs()
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
	levelOff := make([]uint32, 1, len(sys.Levels)+1)
	levelCons := make([]uint32, 0, len(rs))
	hintLevelOff := make([]uint32, 1, len(sys.Levels)+1)
	hintLevel := make([]uint32, 0, len(ha.ids))
	for _, l := range sys.Levels {
		for _, iID := range l {
			if to := instTo[iID]; to&isHint != 0 {
				hintLevel = append(hintLevel, to&^isHint)
			} else {
				levelCons = append(levelCons, to)
			}
		}
		levelOff = append(levelOff, uint32(len(levelCons)))
		hintLevelOff = append(hintLevelOff, uint32(len(hintLevel)))
	}
	nbPublic, nbSecret := sys.GetNbPublicVariables(), sys.GetNbSecretVariables()
	nbWires := nbPublic + nbSecret + sys.NbInternalVariables
	if len(wires) == 0 || len(levelCons) == 0 || len(sys.Coefficients) == 0 {
		return nil, nil
	}
	out := map[int]*deviceSolver{}
	for _, dev := range devs {
		if _, ok := out[dev]; ok {
			continue
		}
		var h C.gg_r1cs_t
		err := onDevice(dev, func() error {
			if C.gg_r1cs_create(C.size_t(nbWires), C.size_t(len(rs)),
				(*C.uint32_t)(unsafe.Pointer(&off[0])), (*C.uint32_t)(unsafe.Pointer(&wires[0])),
				(*C.uint32_t)(unsafe.Pointer(&coeffs[0])), unsafe.Pointer(&sys.Coefficients[0]),
				C.size_t(len(sys.Coefficients)), (*C.uint32_t)(unsafe.Pointer(&levelOff[0])),
				(*C.uint32_t)(unsafe.Pointer(&levelCons[0])), C.size_t(len(sys.Levels)), &h) != C.GG_OK {
				return lastError()
			}
			// the library rejects a witness of another size too (a second line of defence)
			if C.gg_r1cs_set_inputs(h, C.size_t(nbPublic), C.size_t(nbSecret)) != C.GG_OK {
				C.gg_r1cs_release(h)
				return lastError()
			}
			if len(ha.ids) > 0 && C.gg_r1cs_set_hints(h, C.size_t(len(ha.ids)), u32p(ha.ids), u32p(ha.inOff),
				u32p(ha.exprOff), u32p(ha.wires), u32p(ha.coeffs), u32p(ha.outStart), u32p(ha.outEnd),
				u32p(hintLevelOff), u32p(hintLevel), C.size_t(len(sys.Levels))) != C.GG_OK {
				C.gg_r1cs_release(h)
				return lastError()
			}
			return nil
		})
		if err != nil {
			for _, ds := range out {
				ds.release()
			}
			return nil, err
		}
		out[dev] = &deviceSolver{h: h, nbWires: nbWires, nbCons: len(rs), nbInputs: nbPublic - 1 + nbSecret}
	}
	return out, nil
}

// solve runs the levels on the GPU and returns the device pointers of W, A, B, C
// (valid until the next solve on this solver).
func (d *deviceSolver) solve(fullWitness witness.Witness) (w, a, b, c unsafe.Pointer, err error) {
	vec, ok := fullWitness.Vector().(fr.Vector)
	if !ok {
		return nil, nil, nil, nil, fmt.Errorf("gnark_amd: witness is not a bn254 fr.Vector")
	}
	if len(vec) != d.nbInputs { // newSolver (solver.go:71-76)
		return nil, nil, nil, nil, fmt.Errorf("invalid witness size, got %d, expected %d", len(vec), d.nbInputs)
	}
	var in unsafe.Pointer
	if len(vec) > 0 {
		in = unsafe.Pointer(&vec[0])
	}
	var bad C.int64_t
	if rc := C.gg_r1cs_solve(d.h, in, C.size_t(len(vec)), 0, nil, nil, nil, nil, 1, &bad); rc != C.GG_OK {
		if rc == C.GG_ERR_UNSATISFIED {
			return nil, nil, nil, nil, fmt.Errorf("constraint #%d is not satisfied: %w", int64(bad), lastError())
		}
		return nil, nil, nil, nil, lastError()
	}
	if C.gg_r1cs_solution_dev(d.h, &w, &a, &b, &c) != C.GG_OK {
		return nil, nil, nil, nil, lastError()
	}
	return w, a, b, c, nil
}

func (d *deviceSolver) release() {
	if d != nil && d.h != nil {
		C.gg_r1cs_release(d.h)
		d.h = nil
	}
}

// EC-NTT (ecntt.hip): the inverse DFT of a vector of G1 points, shared with the
// PlonK Setup (plonk_setup.hip), which turns the canonical SRS into the Lagrange
// one with it (backend/plonk/bls12-381/setup.go:134, kzg.ToLagrangeG1).
#pragma once
#include "common.h"

namespace gg {
namespace ecntt {

// omega_mont of exact order 2^log_n in the curve's scalar field, 1 <= log_n <= 27
// (GG_ERR_INVALID_ARG otherwise); host only
void check_args(int curve, int log_n, const void* omega_mont);

// out_dev[i] = (1/n) sum_j omega^(-ij) in_dev[j], affine points of `curve` in
// HBM (may alias), enqueued on st and waited for.  ms (nullable): [0] the
// stages (events), [1] the normalisation to affine.
void to_lagrange_dev(int curve, int log_n, const void* omega_mont, const void* in_dev, void* out_dev, hipStream_t st,
                     double* ms);

inline size_t point_bytes(int curve) { return curve == GG_CURVE_BN254 ? 64 : 96; }

}  // namespace ecntt
}  // namespace gg

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

// The same over G2 points (ecntt_g2.hip): 128 B on BN254, 192 B on BLS12-381.
// The BLS12-381 point loops run over Called<Fp2Bls> (pairing.cuh).
void to_lagrange_g2_dev(int curve, int log_n, const void* omega_mont, const void* in_dev, void* out_dev,
                        hipStream_t st, double* ms);

inline size_t point_bytes_g2(int curve) { return 2 * point_bytes(curve); }

// the operands of gg_kzg_to_lagrange_g1 / _g2: host or device, possibly one buffer.
// run(in_dev, out_dev) transforms in HBM and waits for st.
template <class Run>
inline void host_or_device(size_t bytes, const void* in, int in_on_device, void* out, int out_on_device, hipStream_t st,
                           Run run) {
    DevBuf dout;
    const void* din = in;
    void* dst = out;
    if (!out_on_device) {
        dout.alloc(bytes);
        dst = dout.p;
    }
    if (!in_on_device) {
        // a host input goes straight into the output buffer: the transform is in place
        GG_HIP(hipMemcpyAsync(dst, in, bytes, hipMemcpyHostToDevice, st));
        din = dst;
    }
    run(din, dst);
    if (!out_on_device) {
        GG_HIP(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
    }
}

}  // namespace ecntt
}  // namespace gg

// BN254 pairing kernels: the templates of pairing.cuh over Bn254Tower.
//
// Shape: one lane per product of pairings, 64-lane blocks.  A GT element is 96
// dwords; f, the G2 accumulators and a product temporary do not fit 256 VGPRs,
// so the Fp12-level routines of pairing.cuh are real calls and their operands
// live in the lane's stack frame (scratch); the Fp2 products underneath stay in
// registers.  Figures per kernel: DESIGN.md §4 "Groth16 Verify",
// profiles/r10_groth16_verify.md.
//
//   k_pairing      n products of k pairs (variable G2 operands)
//   k_g1_check / k_g2_check   curve and r-torsion membership
// and the host's hash to the scalar field (expand_message_xmd48, which the
// verifiers of both curves share).  BLS12-381: pairing_bls.hip.
// Every argument is validated on the host before the first device call.
#include "common.h"
#include "pairing.cuh"
#include "pairing_host.h"
#include "pairing_run.h"
#include "sha256.h"
#include <cstring>

namespace gg {
namespace pairing {

using Tw = Bn254Tower;
using GT = Fp12<Tw>;
static_assert(sizeof(GT) == GG_GT_BYTES, "E12 layout");

__global__ void __launch_bounds__(64) k_pairing(size_t n, int k, const G1Affine* g1, const G2Affine* g2, GT* out,
                                                uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GT f = pairing_product<Tw>(k, g1 + i * (size_t)k, g2 + i * (size_t)k);
    if (out) out[i] = f;
    if (ok) ok[i] = f.is_one() ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_g1_check(size_t n, const G1Affine* p, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g1_check<Tw>(p[i]);
}
__global__ void __launch_bounds__(64) k_g2_check(size_t n, const G2Affine* q, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g2_check<Tw>(q[i]);
}

// RFC 9380 5.3.1 expand_message_xmd, SHA-256, 48 bytes (pairing_host.h)
void expand_message_xmd48(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len, uint8_t out[64]) {
    const uint8_t dl = (uint8_t)dst_len;
    uint8_t b0[32], bi[32];
    {
        const uint8_t zpad[64] = {0};
        const uint8_t tail[3] = {0, 48, 0};  // l_i_b_str (2 bytes), then I2OSP(0, 1)
        Sha256 h;
        h.update(zpad, 64);
        if (len) h.update(msg, len);
        h.update(tail, 3);
        if (dst_len) h.update(dst, dst_len);
        h.update(&dl, 1);
        h.final(b0);
    }
    memset(bi, 0, 32);
    for (uint8_t i = 1; i <= 2; i++) {
        uint8_t x[32];
        for (int t = 0; t < 32; t++) x[t] = b0[t] ^ bi[t];
        Sha256 h;
        h.update(x, 32);
        h.update(&i, 1);
        if (dst_len) h.update(dst, dst_len);
        h.update(&dl, 1);
        h.final(bi);
        memcpy(out + 32 * (i - 1), bi, 32);
    }
}

}  // namespace pairing
}  // namespace gg

using namespace gg;
using namespace gg::pairing;

extern "C" int gg_pairing_bn254(size_t n, int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, gt_out, "gt_out");
    run_pairing<GT, G1Affine, G2Affine>(k_pairing, n, k, g1, g2, gt_out, nullptr);
    GG_CAPI_END
}
extern "C" int gg_pairing_check_bn254(size_t n, int k, const void* g1, const void* g2, uint8_t* ok_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, ok_out, "ok_out");
    run_pairing<GT, G1Affine, G2Affine>(k_pairing, n, k, g1, g2, nullptr, ok_out);
    GG_CAPI_END
}
extern "C" int gg_pairing_bn254_host(size_t n, int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, gt_out, "gt_out");
    const G1Affine* a = (const G1Affine*)g1;
    const G2Affine* b = (const G2Affine*)g2;
    for (size_t i = 0; i < n; i++) {
        const GT f = pairing_product<Tw>(k, a + i * (size_t)k, b + i * (size_t)k);
        memcpy((char*)gt_out + i * sizeof(GT), &f, sizeof(GT));
    }
    GG_CAPI_END
}
extern "C" int gg_g1_check_bn254(size_t n, const void* g1, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g1, "g1", flags_out);
    run_check<G1Affine>(n, g1, flags_out, k_g1_check, 256);
    GG_CAPI_END
}
extern "C" int gg_g2_check_bn254(size_t n, const void* g2, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g2, "g2", flags_out);
    run_check<G2Affine>(n, g2, flags_out, k_g2_check, 64);
    GG_CAPI_END
}
extern "C" int gg_hash_to_field_bn254(const void* msg, size_t len, const void* dst, size_t dst_len, void* out32) {
    GG_CAPI_BEGIN
    GG_CHECK(msg || !len, GG_ERR_INVALID_ARG, "null argument: msg");
    GG_CHECK(dst || !dst_len, GG_ERR_INVALID_ARG, "null argument: dst");
    GG_CHECK(out32, GG_ERR_INVALID_ARG, "null argument: out32");
    GG_CHECK(dst_len <= 255, GG_ERR_INVALID_ARG, "dst_len must be <= 255 (expand_message_xmd)");
    const Fr h = hash_to_field<Fr>((const uint8_t*)msg, len, (const uint8_t*)dst, dst_len);
    memcpy(out32, &h, 32);
    GG_CAPI_END
}

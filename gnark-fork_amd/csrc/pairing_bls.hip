// BLS12-381 pairing kernels: the templates of pairing.cuh over Bls12381Tower.
//
// Shape: the one of the BN254 kernels (pairing.hip).  One lane per product of
// pairings, 64-lane blocks; a GT element is 144 dwords, so the Fp12-level
// routines are real calls and their operands live in the lane's stack frame
// (scratch); the Fp2 products underneath stay in registers.  Figures per
// kernel: DESIGN.md §4 "BLS12-381 tower", profiles/r12_bls12_381_pairing.md.
//
//   k_pairing_bls      n products of k pairs (variable G2 operands)
//   k_g1_check_bls     curve, then r P = inf by double-and-add (cofactor != 1)
//   k_g2_check_bls     twist, then r Q = inf
// Every argument is validated on the host before the first device call.
#include "common.h"
#include "pairing.cuh"
#include "pairing_run.h"
#include <cstring>
#include <vector>

namespace gg {
namespace pairing {

using TwB = Bls12381Tower;
using GTB = Fp12<TwB>;
using LineB = Line<TwB>;
using G1B = Affine<FpBls>;
using G2B = Affine<Fp2Bls>;
constexpr int kLinesB = line_count<TwB>();
static_assert(sizeof(GTB) == GG_GT_BYTES_BLS12_381, "E12 layout");
static_assert(sizeof(G1B) == 96 && sizeof(G2B) == 192, "point layout");
static_assert(kLinesB == 68, "63 doublings + 5 additions");

__global__ void __launch_bounds__(64) k_pairing_bls(size_t n, int k, const G1B* g1, const G2B* g2, GTB* out,
                                                    uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GTB f = pairing_product<TwB>(k, g1 + i * (size_t)k, g2 + i * (size_t)k);
    if (out) out[i] = f;
    if (ok) ok[i] = f.is_one() ? 1 : 0;
}
__global__ void __launch_bounds__(64) k_g1_check_bls(size_t n, const G1B* p, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g1_check<TwB>(p[i]);
}
__global__ void __launch_bounds__(64) k_g2_check_bls(size_t n, const G2B* q, uint8_t* flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (uint8_t)g2_check<TwB>(q[i]);
}

}  // namespace pairing
}  // namespace gg

using namespace gg;
using namespace gg::pairing;

extern "C" int gg_pairing_bls12_381(size_t n, int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, gt_out, "gt_out");
    run_pairing<GTB, G1B, G2B>(k_pairing_bls, n, k, g1, g2, gt_out, nullptr);
    GG_CAPI_END
}
extern "C" int gg_pairing_check_bls12_381(size_t n, int k, const void* g1, const void* g2, uint8_t* ok_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, ok_out, "ok_out");
    run_pairing<GTB, G1B, G2B>(k_pairing_bls, n, k, g1, g2, nullptr, ok_out);
    GG_CAPI_END
}
extern "C" int gg_pairing_bls12_381_host(size_t n, int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, gt_out, "gt_out");
    const G1B* a = (const G1B*)g1;
    const G2B* b = (const G2B*)g2;
    for (size_t i = 0; i < n; i++) {
        const GTB f = pairing_product<TwB>(k, a + i * (size_t)k, b + i * (size_t)k);
        memcpy((char*)gt_out + i * sizeof(GTB), &f, sizeof(GTB));
    }
    GG_CAPI_END
}
extern "C" int gg_pairing_bls12_381_table_host(int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    GG_CHECK(k >= 1 && k <= 3, GG_ERR_INVALID_ARG, "k must be 1, 2 or 3 (pairs of one Miller loop)");
    GG_CHECK(g1, GG_ERR_INVALID_ARG, "null argument: g1");
    GG_CHECK(g2, GG_ERR_INVALID_ARG, "null argument: g2");
    GG_CHECK(gt_out, GG_ERR_INVALID_ARG, "null argument: gt_out");
    G1B p[3];
    G2Src<TwB> s[3];
    std::vector<LineB> lines((size_t)3 * kLinesB);
    for (int t = 0; t < k; t++) {
        G2B q;
        memcpy(&p[t], (const char*)g1 + (size_t)t * sizeof(G1B), sizeof(G1B));
        memcpy(&q, (const char*)g2 + (size_t)t * sizeof(G2B), sizeof(G2B));
        line_table<TwB>(q, lines.data() + (size_t)t * kLinesB);
        s[t].tab = lines.data() + (size_t)t * kLinesB;
        s[t].pos = 0;
        s[t].skip = p[t].is_inf() || q.is_inf();
    }
    GTB f = GTB::one();
    if (k == 3) miller_loop<TwB, 3>(f, p, s);
    else if (k == 2) miller_loop<TwB, 2>(f, p, s);
    else miller_loop<TwB, 1>(f, p, s);
    for (int t = 0; t < k; t++)
        GG_CHECK(s[t].skip || s[t].pos == kLinesB, GG_ERR_INTERNAL,
                 "the loop read " + std::to_string(s[t].pos) + " lines of a table of " + std::to_string(kLinesB));
    f = final_exp(f);
    memcpy(gt_out, &f, sizeof(GTB));
    GG_CAPI_END
}
extern "C" int gg_g1_check_bls12_381(size_t n, const void* g1, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g1, "g1", flags_out);
    run_check<G1B>(n, g1, flags_out, k_g1_check_bls, 64);
    GG_CAPI_END
}
extern "C" int gg_g2_check_bls12_381(size_t n, const void* g2, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    check_points_args(n, g2, "g2", flags_out);
    run_check<G2B>(n, g2, flags_out, k_g2_check_bls, 64);
    GG_CAPI_END
}

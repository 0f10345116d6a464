// BN254 pairing kernels and Groth16 Verify for batches of proofs under one
// verifying key (backend/groth16/bn254/verify.go:43-140).
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
//   k_vk_table     T[t][w][j] = j 2^(8w) K[t + 1] (XYZZ, then normalised to affine
//                  by comb.h's batch normalisation): the public-input sum's table
//   k_pub_partial  one lane per (proof, slice of 8 public inputs): 32 mixed
//                  additions per scalar, no doubling; exact for 0 and r - 1
//   k_g16_prep     per proof: the point checks, kSum, the folded commitment
//   k_g16_pair     per proof: the Pedersen check, then the 3-pair Miller loop
//                  with the key's line tables for -delta and -gamma, the final
//                  exponentiation and the comparison with e(alpha, beta)^m
// The commitment hashes and the folding challenge run on the host.
// Every argument is validated on the host before the first device call.
#include "common.h"
#include "pairing.cuh"
#include "pairing_host.h"
#include "pairing_run.h"
#include "comb.h"
#include "sha256.h"
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace gg {
namespace pairing {

using Tw = Bn254Tower;
using GT = Fp12<Tw>;
using LineT = Line<Tw>;
constexpr int kLines = line_count<Tw>();
constexpr int kSlice = 8;  // public inputs per lane of k_pub_partial
static_assert(sizeof(GT) == GG_GT_BYTES, "E12 layout");
static_assert(sizeof(LineT) == 192, "line layout");

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

// lane (t, w): the 256 multiples of 2^(8w) K[t + 1]
__global__ void __launch_bounds__(64) k_vk_table(const G1Affine* K, size_t nsc, G1Xyzz* out) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nsc * 32) return;
    const size_t t = id >> 5;
    const int w = (int)(id & 31);
    G1Xyzz b = G1Xyzz::from_affine(K[t + 1]);
    for (int s = 0; s < 8 * w; s++) b = xyzz_dbl(b);
    G1Xyzz* o = out + id * 256;
    o[0] = G1Xyzz::inf();
    G1Xyzz acc = b;
    for (int j = 1; j < 256; j++) {
        o[j] = acc;
        acc = xyzz_add(acc, b);
    }
}
// scalar t of proof p: the public witness, then the commitment hashes
__device__ __forceinline__ Fr pub_scalar(const Fr* wit, const Fr* hashes, size_t p, size_t t, size_t nw, size_t nc) {
    return t < nw ? wit[p * nw + t] : hashes[p * nc + (t - nw)];
}
__global__ void __launch_bounds__(256) k_pub_partial(size_t n, size_t nsc, size_t nw, size_t nc, size_t nslices,
                                                     const G1Affine* table, const Fr* wit, const Fr* hashes,
                                                     G1Xyzz* part) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n * nslices) return;
    const size_t p = id / nslices, s = id - p * nslices;
    const size_t t1 = (s + 1) * kSlice < nsc ? (s + 1) * kSlice : nsc;
    G1Xyzz acc = G1Xyzz::inf();
    for (size_t t = s * kSlice; t < t1; t++) {
        Fr x = from_mont(pub_scalar(wit, hashes, p, t, nw, nc));
        for (int w = 0; w < 32; w++) {  // the low byte, then the scalar moves down by 8 bits
            const uint32_t j = x.v[0] & 0xffu;
            if (j) xyzz_madd_inplace(acc, table[(t * 32 + (size_t)w) * 256 + j]);
#pragma unroll
            for (int q = 0; q < 7; q++) x.v[q] = (x.v[q] >> 8) | (x.v[q + 1] << 24);
            x.v[7] >>= 8;
        }
    }
    part[id] = acc;
}

struct ProofBytes {
    G1Affine ar;
    G2Affine bs;
    G1Affine krs;
};
static_assert(sizeof(ProofBytes) == 256, "proof layout");

__device__ __forceinline__ G1Affine xyzz_to_affine(const G1Xyzz& p) {
    if (p.is_inf()) return G1Affine::inf();
    const Fp i3 = inverse(p.zzz);
    return G1Affine{p.x * sqr(p.zz * i3), p.y * i3};
}
// k a for a canonical scalar in global memory (8 words)
__device__ __noinline__ G1Jac g1_mul_words(const G1Jac& a, const uint32_t* k) {
    G1Jac acc = G1Jac::inf();
    for (int wd = 7; wd >= 0; wd--) {
        const uint32_t word = k[wd];
        for (int b = 31; b >= 0; b--) {
            acc = jac_dbl(acc);
            if ((word >> b) & 1) acc = jac_add(acc, a);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(64) k_g16_prep(size_t n, size_t nc, size_t nslices, const ProofBytes* proofs,
                                                 const G1Affine* cmts, const G1Affine* poks, const G1Affine* K,
                                                 const G1Xyzz* part, const uint32_t* chal, G1Affine* ksum,
                                                 G1Affine* folded, uint8_t* status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ProofBytes& pr = proofs[i];
    bool bad = g1_check<Tw>(pr.ar) != 0 || g1_check<Tw>(pr.krs) != 0;
    for (size_t j = 0; j < nc; j++) bad = bad || g1_check<Tw>(cmts[i * nc + j]) != 0;
    if (nc) bad = bad || g1_check<Tw>(poks[i]) != 0;
    if (!bad) bad = g2_check<Tw>(pr.bs) != 0;
    if (bad) {
        status[i] = GG_VERIFY_SUBGROUP;
        return;
    }
    G1Xyzz acc = G1Xyzz::from_affine(K[0]);
    for (size_t s = 0; s < nslices; s++) xyzz_add_inplace(acc, part[i * nslices + s]);
    for (size_t j = 0; j < nc; j++) {
        const G1Affine c = cmts[i * nc + j];
        if (!c.is_inf()) xyzz_madd_inplace(acc, c);
    }
    ksum[i] = xyzz_to_affine(acc);
    if (nc) {  // sum_j r^j C_j by Horner (pedersen.FoldCommitments; one commitment: itself)
        G1Jac f = G1Jac::from_affine(cmts[i * nc + nc - 1]);
        for (size_t j = nc - 1; j-- > 0;) f = jac_add(g1_mul_words(f, chal + 8 * i), G1Jac::from_affine(cmts[i * nc + j]));
        folded[i] = jac_to_affine(f);
    }
    status[i] = GG_VERIFY_OK;
}

struct VkDev {
    const LineT *delta_neg, *gamma_neg, *ped_g, *ped_gs;
    const GT* e;
};
__global__ void __launch_bounds__(64) k_g16_pair(size_t n, size_t nc, const ProofBytes* proofs, const G1Affine* poks,
                                                 const G1Affine* ksum, const G1Affine* folded, VkDev vk,
                                                 uint8_t* status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] != GG_VERIFY_OK) return;
    G1Affine p[3];
    G2Src<Tw> s[3];
    if (nc) {  // e(folded, G) e(pok, GRootSigmaNeg) == 1
        p[0] = folded[i];
        p[1] = poks[i];
        s[0].tab = vk.ped_g;
        s[0].skip = p[0].is_inf();
        s[1].tab = vk.ped_gs;
        s[1].skip = p[1].is_inf();
        GT f = GT::one();
        miller_loop<Tw, 2>(f, p, s);
        if (!final_exp(f).is_one()) {
            status[i] = GG_VERIFY_PEDERSEN;
            return;
        }
    }
    const ProofBytes& pr = proofs[i];
    p[0] = pr.krs;
    p[1] = pr.ar;
    p[2] = ksum[i];
    s[0].tab = vk.delta_neg;
    s[0].pos = 0;
    s[0].skip = p[0].is_inf();
    src_init<Tw>(s[1], pr.bs, nullptr, p[1].is_inf());
    s[2].tab = vk.gamma_neg;
    s[2].pos = 0;
    s[2].skip = p[2].is_inf();
    GT f = GT::one();
    miller_loop<Tw, 3>(f, p, s);
    status[i] = final_exp(f) == *vk.e ? GG_VERIFY_OK : GG_VERIFY_PAIRING;
}

// ------------------------------------------------------------------ host side
static void run_pairing(size_t n, int k, const void* g1, const void* g2, void* gt_out, uint8_t* ok_out) {
    Stream st;
    DevBuf b1, b2;
    const size_t np = n * (size_t)k;
    const G1Affine* d1 = (const G1Affine*)to_device(g1, np * sizeof(G1Affine), b1, st.s);
    const G2Affine* d2 = (const G2Affine*)to_device(g2, np * sizeof(G2Affine), b2, st.s);
    OutBuf o;
    if (gt_out) o.init(gt_out, n * sizeof(GT));
    else o.init(ok_out, n);
    hipLaunchKernelGGL(k_pairing, dim3(grid_for(n, 64)), dim3(64), 0, st.s, n, k, d1, d2,
                       gt_out ? (GT*)o.dev : nullptr, gt_out ? nullptr : (uint8_t*)o.dev);
    GG_HIP(hipGetLastError());
    o.finish(st.s);
}

// big-endian bytes mod r, Montgomery form (Horner over the bytes)
static Fr fr_from_be(const uint8_t* b, size_t n) {
    Fr m256 = Fr::zero(), acc = Fr::zero();
    m256.v[0] = 256;
    m256 = to_mont(m256);
    for (size_t i = 0; i < n; i++) {
        Fr d = Fr::zero();
        d.v[0] = b[i];
        acc = acc * m256 + to_mont(d);
    }
    return acc;
}
template <class F>
static void fe_to_be(const F& mont, uint8_t out[32]) {
    const F c = from_mont(mont);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(c.v[7 - i / 4] >> (8 * (3 - i % 4)));
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
Fr hash_to_field(const uint8_t* msg, size_t len, const uint8_t* dst, size_t dst_len) {
    uint8_t out[64];
    expand_message_xmd48(msg, len, dst, dst_len, out);
    return fr_from_be(out, 48);
}
static const uint8_t kCommitmentDst[] = "bsb22-commitment";  // constraint/commitment.go:7

}  // namespace pairing
}  // namespace gg

using namespace gg;
using namespace gg::pairing;

struct gg_groth16_vk {
    int device = 0;
    size_t n_K = 0, nb_public = 0, nc = 0;
    std::vector<uint32_t> coff, cidx;
    DevBuf K, table, lines, e;  // lines: -delta, -gamma, G, GRootSigmaNeg (kLines each)
    std::mutex mu;              // one batch at a time per key: the buffers below are the key's
    hipStream_t st = nullptr;
    DevBuf proofs, cmts, poks, wit, hashes, chal, part, ksum, folded, status;
    ~gg_groth16_vk() {
        if (st) (void)hipStreamDestroy(st);
    }
};

extern "C" int gg_pairing_bn254(size_t n, int k, const void* g1, const void* g2, void* gt_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, gt_out, "gt_out");
    run_pairing(n, k, g1, g2, gt_out, nullptr);
    GG_CAPI_END
}
extern "C" int gg_pairing_check_bn254(size_t n, int k, const void* g1, const void* g2, uint8_t* ok_out) {
    GG_CAPI_BEGIN
    check_pairing_args(n, k, g1, g2, ok_out, "ok_out");
    run_pairing(n, k, g1, g2, nullptr, ok_out);
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
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(g1, GG_ERR_INVALID_ARG, "null argument: g1");
    GG_CHECK(flags_out, GG_ERR_INVALID_ARG, "null argument: flags_out");
    run_check<G1Affine>(n, g1, flags_out, k_g1_check, 256);
    GG_CAPI_END
}
extern "C" int gg_g2_check_bn254(size_t n, const void* g2, uint8_t* flags_out) {
    GG_CAPI_BEGIN
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(g2, GG_ERR_INVALID_ARG, "null argument: g2");
    GG_CHECK(flags_out, GG_ERR_INVALID_ARG, "null argument: flags_out");
    run_check<G2Affine>(n, g2, flags_out, k_g2_check, 64);
    GG_CAPI_END
}
extern "C" int gg_hash_to_field_bn254(const void* msg, size_t len, const void* dst, size_t dst_len, void* out32) {
    GG_CAPI_BEGIN
    GG_CHECK(msg || !len, GG_ERR_INVALID_ARG, "null argument: msg");
    GG_CHECK(dst || !dst_len, GG_ERR_INVALID_ARG, "null argument: dst");
    GG_CHECK(out32, GG_ERR_INVALID_ARG, "null argument: out32");
    GG_CHECK(dst_len <= 255, GG_ERR_INVALID_ARG, "dst_len must be <= 255 (expand_message_xmd)");
    const Fr h = hash_to_field((const uint8_t*)msg, len, (const uint8_t*)dst, dst_len);
    memcpy(out32, &h, 32);
    GG_CAPI_END
}

extern "C" int gg_groth16_vk_create(int curve, const void* alpha1, const void* beta2, const void* gamma2,
                                    const void* delta2, const void* K, size_t n_K, size_t nb_public,
                                    const void* ped_g, const void* ped_g_root_sigma_neg,
                                    const uint32_t* committed_off, const uint32_t* committed_idx, int n_commitments,
                                    gg_groth16_vk_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out, GG_ERR_INVALID_ARG, "null argument: out");
    *out = nullptr;
    GG_CHECK(curve == GG_CURVE_BN254, GG_ERR_UNSUPPORTED,
             "curve " + std::to_string(curve) + " is not supported: Groth16 Verify has a BN254 pairing only");
    GG_CHECK(alpha1, GG_ERR_INVALID_ARG, "null argument: alpha1");
    GG_CHECK(beta2, GG_ERR_INVALID_ARG, "null argument: beta2");
    GG_CHECK(gamma2, GG_ERR_INVALID_ARG, "null argument: gamma2");
    GG_CHECK(delta2, GG_ERR_INVALID_ARG, "null argument: delta2");
    GG_CHECK(K, GG_ERR_INVALID_ARG, "null argument: K");
    GG_CHECK(nb_public >= 1, GG_ERR_INVALID_ARG, "nb_public must be >= 1 (it counts the ONE wire)");
    GG_CHECK(n_commitments >= 0, GG_ERR_INVALID_ARG, "n_commitments must be >= 0");
    const size_t nc = (size_t)n_commitments;
    GG_CHECK(n_K == nb_public + nc, GG_ERR_INVALID_ARG,
             "n_K = " + std::to_string(n_K) + " but nb_public + n_commitments = " + std::to_string(nb_public + nc));
    GG_CHECK(n_K <= GG_VERIFY_MAX_K, GG_ERR_INVALID_ARG,
             "n_K = " + std::to_string(n_K) + " exceeds GG_VERIFY_MAX_K = " + std::to_string(GG_VERIFY_MAX_K));
    std::unique_ptr<gg_groth16_vk> vk(new gg_groth16_vk);
    if (nc) {
        GG_CHECK(ped_g, GG_ERR_INVALID_ARG, "null argument: ped_g");
        GG_CHECK(ped_g_root_sigma_neg, GG_ERR_INVALID_ARG, "null argument: ped_g_root_sigma_neg");
        GG_CHECK(committed_off, GG_ERR_INVALID_ARG, "null argument: committed_off");
        GG_CHECK(committed_off[0] == 0, GG_ERR_INVALID_ARG, "committed_off[0] must be 0");
        for (size_t j = 0; j < nc; j++)
            GG_CHECK(committed_off[j] <= committed_off[j + 1], GG_ERR_INVALID_ARG, "committed_off must not decrease");
        GG_CHECK(committed_idx || !committed_off[nc], GG_ERR_INVALID_ARG, "null argument: committed_idx");
        for (size_t j = 0; j < nc; j++)
            for (uint32_t t = committed_off[j]; t < committed_off[j + 1]; t++)
                GG_CHECK(committed_idx[t] >= 1 && committed_idx[t] < nb_public + j, GG_ERR_INVALID_ARG,
                         "committed index " + std::to_string(committed_idx[t]) + " of commitment " + std::to_string(j) +
                             " out of range [1, " + std::to_string(nb_public + j) + ")");
        vk->coff.assign(committed_off, committed_off + nc + 1);
        vk->cidx.assign(committed_idx, committed_idx + committed_off[nc]);
    }
    G2Affine q[4];
    memcpy(&q[0], delta2, sizeof(G2Affine));
    memcpy(&q[1], gamma2, sizeof(G2Affine));
    GG_CHECK(!q[0].is_inf(), GG_ERR_INVALID_ARG, "delta2 is the point at infinity");
    GG_CHECK(!q[1].is_inf(), GG_ERR_INVALID_ARG, "gamma2 is the point at infinity");
    q[0] = neg(q[0]);
    q[1] = neg(q[1]);
    int nq = 2;
    if (nc) {
        memcpy(&q[2], ped_g, sizeof(G2Affine));
        memcpy(&q[3], ped_g_root_sigma_neg, sizeof(G2Affine));
        GG_CHECK(!q[2].is_inf(), GG_ERR_INVALID_ARG, "ped_g is the point at infinity");
        GG_CHECK(!q[3].is_inf(), GG_ERR_INVALID_ARG, "ped_g_root_sigma_neg is the point at infinity");
        nq = 4;
    }
    vk->n_K = n_K;
    vk->nb_public = nb_public;
    vk->nc = nc;
    // the fixed operands' lines, by the templates the kernels run
    std::vector<LineT> lines((size_t)4 * kLines);
    for (int t = 0; t < nq; t++) line_table<Tw>(q[t], lines.data() + (size_t)t * kLines);
    // ---- device
    GG_HIP(hipGetDevice(&vk->device));
    GG_HIP(hipStreamCreateWithFlags(&vk->st, hipStreamNonBlocking));
    hipStream_t st = vk->st;
    vk->lines.alloc(lines.size() * sizeof(LineT));
    GG_HIP(hipMemcpyAsync(vk->lines.p, lines.data(), vk->lines.bytes, hipMemcpyHostToDevice, st));
    vk->K.alloc(n_K * sizeof(G1Affine));
    GG_HIP(hipMemcpyAsync(vk->K.p, K, vk->K.bytes, hipMemcpyHostToDevice, st));
    DevBuf ab(sizeof(G1Affine) + sizeof(G2Affine));
    GG_HIP(hipMemcpyAsync(ab.p, alpha1, sizeof(G1Affine), hipMemcpyHostToDevice, st));
    GG_HIP(hipMemcpyAsync((char*)ab.p + sizeof(G1Affine), beta2, sizeof(G2Affine), hipMemcpyHostToDevice, st));
    vk->e.alloc(sizeof(GT));
    hipLaunchKernelGGL(k_pairing, dim3(1), dim3(64), 0, st, (size_t)1, 1, (const G1Affine*)ab.p,
                       (const G2Affine*)((char*)ab.p + sizeof(G1Affine)), vk->e.as<GT>(), (uint8_t*)nullptr);
    GG_HIP(hipGetLastError());
    const size_t nsc = n_K - 1;
    DevBuf cur, prefix;
    if (nsc) {
        const size_t ne = nsc * 32 * 256;
        cur.alloc(ne * sizeof(G1Xyzz));
        prefix.alloc(ne * sizeof(Fp));
        vk->table.alloc(ne * sizeof(G1Affine));
        hipLaunchKernelGGL(k_vk_table, dim3(grid_for(nsc * 32, 64)), dim3(64), 0, st, vk->K.as<G1Affine>(), nsc,
                           cur.as<G1Xyzz>());
        GG_HIP(hipGetLastError());
        const size_t T = std::min<size_t>(ne, 16384);
        hipLaunchKernelGGL(comb::k_comb_normalize<Fp>, dim3(grid_for(T, 256)), dim3(256), 0, st,
                           (const G1Xyzz*)cur.p, ne, T, prefix.as<Fp>(), vk->table.as<G1Affine>());
        GG_HIP(hipGetLastError());
    }
    GG_WAIT_STREAM(st);
    *out = vk.release();
    GG_CAPI_END
}
extern "C" int gg_groth16_vk_destroy(gg_groth16_vk_t vk) {
    GG_CAPI_BEGIN
    delete vk;
    GG_CAPI_END
}

// host copy of `bytes` at p (p itself when it is host memory)
static const uint8_t* to_host(const void* p, size_t bytes, std::vector<uint8_t>& buf) {
    if (!bytes || !is_device_ptr(p)) return (const uint8_t*)p;
    buf.resize(bytes);
    GG_HIP(hipMemcpy(buf.data(), p, bytes, hipMemcpyDeviceToHost));
    return buf.data();
}

extern "C" int gg_groth16_verify_batch(gg_groth16_vk_t vk, size_t n, const void* proofs, const void* commitments,
                                       const void* poks, const void* public_witness, uint8_t* status_out) {
    GG_CAPI_BEGIN
    GG_CHECK(vk, GG_ERR_INVALID_ARG, "null argument: vk");
    GG_CHECK(n > 0, GG_ERR_INVALID_ARG, "n must be > 0");
    GG_CHECK(n <= ((size_t)1 << 24), GG_ERR_INVALID_ARG, "n exceeds 2^24 proofs per call");
    GG_CHECK(proofs, GG_ERR_INVALID_ARG, "null argument: proofs");
    GG_CHECK(status_out, GG_ERR_INVALID_ARG, "null argument: status_out");
    const size_t nc = vk->nc, nw = vk->nb_public - 1, nsc = vk->n_K - 1;
    GG_CHECK(commitments || !nc, GG_ERR_INVALID_ARG, "null argument: commitments (the key has commitments)");
    GG_CHECK(poks || !nc, GG_ERR_INVALID_ARG, "null argument: poks (the key has commitments)");
    GG_CHECK(public_witness || !nw, GG_ERR_INVALID_ARG, "null argument: public_witness");
    std::lock_guard<std::mutex> lock(vk->mu);
    GG_HIP(hipSetDevice(vk->device));
    hipStream_t st = vk->st;
    // ---- host: the commitment hashes and the folding challenge (verify.go:80-100)
    std::vector<Fr> hashes(n * nc);
    std::vector<uint32_t> chal(nc > 1 ? n * 8 : 0);
    if (nc) {
        std::vector<uint8_t> hb_c, hb_w;
        const G1Affine* C = (const G1Affine*)to_host(commitments, n * nc * sizeof(G1Affine), hb_c);
        const Fr* W = (const Fr*)to_host(public_witness, n * nw * sizeof(Fr), hb_w);
        std::vector<uint8_t> msg, ser(1 + 32 * nc);
        ser[0] = 'r';
        for (size_t i = 0; i < n; i++) {
            for (size_t j = 0; j < nc; j++) {
                const uint32_t t0 = vk->coff[j], t1 = vk->coff[j + 1];
                msg.assign(64 + 32 * (size_t)(t1 - t0), 0);
                const G1Affine& c = C[i * nc + j];
                if (c.is_inf()) {
                    msg[0] = 0x40;  // RawEncoding's infinity flag
                } else {
                    fe_to_be(c.x, msg.data());
                    fe_to_be(c.y, msg.data() + 32);
                }
                for (uint32_t t = t0; t < t1; t++) {
                    const size_t idx = vk->cidx[t] - 1;  // into the witness extended by the earlier hashes
                    fe_to_be(idx < nw ? W[i * nw + idx] : hashes[i * nc + (idx - nw)], msg.data() + 64 + 32 * (t - t0));
                }
                const Fr h = hash_to_field(msg.data(), msg.size(), kCommitmentDst, sizeof(kCommitmentDst) - 1);
                hashes[i * nc + j] = h;
                fe_to_be(h, ser.data() + 1 + 32 * j);
            }
            if (nc > 1) {  // pedersen getChallenge: sha256("r" | hashes) mod r
                uint8_t d[32];
                Sha256::hash(ser.data(), ser.size(), d);
                const Fr r = from_mont(fr_from_be(d, 32));
                memcpy(&chal[8 * i], r.v, 32);
            }
        }
    }
    // ---- device
    const size_t nslices = (nsc + kSlice - 1) / kSlice;
    const ProofBytes* dpr = (const ProofBytes*)to_device(proofs, n * sizeof(ProofBytes), vk->proofs, st);
    const G1Affine* dcm = (const G1Affine*)to_device(commitments, n * nc * sizeof(G1Affine), vk->cmts, st);
    const G1Affine* dpk = (const G1Affine*)to_device(poks, nc ? n * sizeof(G1Affine) : 0, vk->poks, st);
    const Fr* dw = (const Fr*)to_device(public_witness, n * nw * sizeof(Fr), vk->wit, st);
    if (nc) {
        vk->hashes.reserve(hashes.size() * sizeof(Fr));
        GG_HIP(hipMemcpyAsync(vk->hashes.p, hashes.data(), hashes.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
    }
    if (!chal.empty()) {
        vk->chal.reserve(chal.size() * 4);
        GG_HIP(hipMemcpyAsync(vk->chal.p, chal.data(), chal.size() * 4, hipMemcpyHostToDevice, st));
    }
    vk->ksum.reserve(n * sizeof(G1Affine));
    if (nc) vk->folded.reserve(n * sizeof(G1Affine));
    OutBuf so;
    if (is_device_ptr(status_out)) {
        so.dev = status_out;
    } else {
        vk->status.reserve(n);
        so.host = status_out;
        so.dev = vk->status.p;
    }
    so.bytes = n;
    if (nslices) {
        vk->part.reserve(n * nslices * sizeof(G1Xyzz));
        hipLaunchKernelGGL(k_pub_partial, dim3(grid_for(n * nslices, 256)), dim3(256), 0, st, n, nsc, nw, nc, nslices,
                           vk->table.as<G1Affine>(), dw, vk->hashes.as<Fr>(), vk->part.as<G1Xyzz>());
        GG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_g16_prep, dim3(grid_for(n, 64)), dim3(64), 0, st, n, nc, nslices, dpr, dcm, dpk,
                       vk->K.as<G1Affine>(), vk->part.as<G1Xyzz>(), vk->chal.as<uint32_t>(), vk->ksum.as<G1Affine>(),
                       vk->folded.as<G1Affine>(), (uint8_t*)so.dev);
    GG_HIP(hipGetLastError());
    const LineT* L = vk->lines.as<LineT>();
    const VkDev vd{L, L + kLines, L + 2 * kLines, L + 3 * kLines, vk->e.as<GT>()};
    hipLaunchKernelGGL(k_g16_pair, dim3(grid_for(n, 64)), dim3(64), 0, st, n, nc, dpr, dpk,
                       (const G1Affine*)vk->ksum.p, (const G1Affine*)vk->folded.p, vd, (uint8_t*)so.dev);
    GG_HIP(hipGetLastError());
    so.finish(st);
    GG_CAPI_END
}

// Groth16 keys from a powers-of-tau SRS: phase 2 of gnark's MPC setup on the GPU
// (backend/groth16/bn254/mpcsetup/phase2.go:53-210 InitPhase2 / Contribute,
// setup.go:25-97 ExtractKeys, lagrange.go; the same files under bls12-381/).
// Nobody knows tau, alpha or beta, so what groth16_setup.hip does in Fr happens
// here over points.  The result is a gg_g16_setup: gg_groth16_setup_info / _read /
// _timings / _release serve it as they serve gg_groth16_setup's.
//
//   1. Lagrange forms  [L_j]1, [alpha L_j]1, [beta L_j]1, [L_j]2 of the first n
//      points of each SRS part: four EC-NTTs (ecntt.hip, ecntt_g2.hip).
//   2. Transposed system: k_count / k_fill of groth16_setup_common.h, unchanged.
//   3. Coefficients by value: one host pass over the table marks every id as 0,
//      1, 2, -1 or general (this ABI reserves no ids).  A general term is one
//      scalar multiplication; they get a pass of their own (k_gen_mul: one lane
//      per general term, 256 doublings each, every lane of every wave busy) that
//      leaves c * [L_j] as an XYZZ point for the accumulation.  The accumulation's
//      lanes then only add: a wave never waits for a multiplication.
//   4. Accumulate, the chunk / round scheme of Setup over XYZZ items
//      (acc_rounds): 0 skips, 1 / -1 are one mixed addition, 2 is two, a general
//      term adds its product.  Three runs: keys (L, R, O) x [L_j]1 -> A, B1, C;
//      keys (L, R) x ([beta L_j]1, [alpha L_j]1) -> bA, aB; keys R x [L_j]2 -> B2.
//      The additions are complete (xyzz_madd / xyzz_add handle P + P and P - P).
//   5. K[w] = bA + aB + C into vk.G1.K (w < nb_public) or pk.G1.K; Z[i] =
//      tau_g1[i + n] - tau_g1[i] bit-reversed; infinity flags and compaction by
//      value; one batch normalisation per output array (comb.h).
//   gg_groth16_setup_contribute: delta1, delta2 *= delta; Z, pk.G1.K *= 1/delta
//      (k_scale: one lane per point, one scalar for all, so no lane diverges).
//
// Over BLS12-381 the G2 kernels run over Called<Fp2Bls> (pairing.cuh): every
// point loop's products are real calls (DESIGN.md §4 "Products as calls in the
// r-torsion loop").
#include "common.h"
#include "field.cuh"
#include "curve.cuh"
#include "comb.h"
#include "ecntt.h"
#include "groth16_setup_common.h"
#include "pairing.cuh"
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gg {
namespace g16m {

using namespace g16s;
using comb::cld;
using comb::cst;

// Items per thread of the accumulation.  An item here is a point addition: 10
// (mixed) to 14 field products and a 64..384-B gather, some hundred times the
// scalar path's one product.  The fixed cost of a thread (a binary search and
// one XYZZ store) is therefore paid back after a few items, and what a long
// chunk buys -- fewer partial sums -- matters less than the lanes it takes away:
// the ONE wire of a 2^20 MiMC system (350 k terms) gives 22 k lanes at 16 and
// 11 k at 32, and the longest chunk is the tail of the launch.  16 keeps a 2^24
// system at 6 rounds.  The kernels below hold one accumulator and one operand
// whatever the chunk, so the registers do not decide it.  Not measured against
// other lengths: the rounds are 1 % of the call (profiles/r15_groth16_mpc_setup.md).
constexpr uint32_t ACC_CHUNK_PTS = 16;
constexpr uint32_t PT_BLOCK = 128;

enum : uint8_t { C_ZERO = 0, C_ONE = 1, C_TWO = 2, C_MINUS_ONE = 3, C_GENERAL = 4 };

using G2Bls = pairing::Called<Fp2Bls>;
static_assert(sizeof(Affine<G2Bls>) == 192 && sizeof(Xyzz<G2Bls>) == 384, "Called<> adds no bytes");

// the three sides' source tables and where each side's entries begin in ent
template <class F>
struct Src {
    const Affine<F>* t[3];
    uint32_t eb[4];
};

// k P, k canonical (8 words, bit 255 clear), P not infinity
template <class F>
__device__ __forceinline__ Xyzz<F> pt_mul(const Affine<F>& p, const uint32_t* k) {
    Xyzz<F> acc = Xyzz<F>::inf();
    for (int i = 254; i >= 0; i--) {
        acc = xyzz_dbl(acc);  // the doubling of infinity is infinity by the formula
        if ((k[i >> 5] >> (i & 31)) & 1u) xyzz_madd_inplace(acc, p);
    }
    return acc;
}

// ---------------------------------------------------------------- general terms
// flag[i] = entry i carries a general coefficient (i < m), flag[m] = 0
__global__ void __launch_bounds__(256) k_gen_flag(const uint2* ent, const uint8_t* ccls, uint32_t m, uint32_t* flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    flag[i] = i < m && ccls[ent[i].y] == C_GENERAL ? 1u : 0u;
}
// glist[g] = the entry of general term g (rank: the exclusive scan of the flags, m + 1 values)
__global__ void __launch_bounds__(256) k_gen_list(const uint32_t* rank, uint32_t m, uint32_t* glist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (rank[i + 1] != rank[i]) glist[rank[i]] = i;
}
// out[g] = coefficient * source point of general term g0 + g, g < cnt
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_gen_mul(Src<F> s, const uint2* ent, const uint32_t* glist, uint32_t g0,
                                                      uint32_t cnt, const uint32_t* kcanon, Xyzz<F>* out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= cnt) return;
    const uint32_t e = glist[g0 + g];
    const uint32_t side = (e >= s.eb[1] ? 1u : 0u) + (e >= s.eb[2] ? 1u : 0u);
    const uint2 en = ent[e];
    const Affine<F> p = cld(s.t[side] + en.x);
    if (p.is_inf()) {
        cst(out + g, Xyzz<F>::inf());
        return;
    }
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = kcanon[8 * (size_t)en.y + i];
    cst(out + g, pt_mul<F>(p, k));
}

// ---------------------------------------------------------------- accumulate
// k_acc of groth16_setup.hip over points: thread i adds chunk c = i - thr_off[k]
// of key k (side side0 + k / nw).  FIRST: items are entries (constraint,
// coefficient id); else the partial sums of the previous round.
template <class F, bool FIRST>
__global__ void __launch_bounds__(PT_BLOCK) k_acc_pts(const uint32_t* prev_off, const uint32_t* thr_off, uint32_t nk,
                                                      uint32_t nthr, uint32_t nw, uint32_t side0, const uint2* ent,
                                                      const uint8_t* ccls, Src<F> s, const uint32_t* rank, uint32_t g0,
                                                      const Xyzz<F>* gen, const Xyzz<F>* psrc, Xyzz<F>* pdst,
                                                      Xyzz<F>* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthr) return;
    uint32_t lo = 0, hi = nk;  // thr_off[lo] <= i < thr_off[hi] (thr_off[nk] = nthr)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (thr_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const uint32_t k = lo;
    const uint32_t c = i - thr_off[k];
    const uint32_t work = thr_off[k + 1] - thr_off[k];
    const uint32_t cnt = pending(prev_off, k, FIRST);
    const uint32_t b0 = c * ACC_CHUNK_PTS;
    const uint32_t m = min(ACC_CHUNK_PTS, cnt - b0);
    const size_t base = (size_t)prev_off[k] + b0;
    Xyzz<F> acc = Xyzz<F>::inf();
    if (FIRST) {
        const Affine<F>* tab = s.t[side0 + k / nw];
        for (uint32_t e = 0; e < m; e++) {
            const uint2 en = ent[base + e];
            const uint8_t cl = ccls[en.y];
            if (cl == C_ZERO) continue;
            if (cl == C_GENERAL) {
                xyzz_add_inplace(acc, cld(gen + (rank[base + e] - g0)));
                continue;
            }
            Affine<F> p = cld(tab + en.x);
            if (p.is_inf()) continue;
            if (cl == C_MINUS_ONE) p.y = -p.y;
            xyzz_madd_inplace(acc, p);
            if (cl == C_TWO) xyzz_madd_inplace(acc, p);
        }
    } else {
        for (uint32_t e = 0; e < m; e++) xyzz_add_inplace(acc, cld(psrc + base + e));
    }
    if (work == 1u) cst(out + k, acc);
    else cst(pdst + i, acc);
}

// ---------------------------------------------------------------- Z, K, flags
// zs[brev(i)] = tau[i + n] - tau[i], i < n - 1 (phase2.go:148-154; brev(i) = n - 1
// only for i = n - 1, the slot the truncation drops)
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_z(const Affine<F>* tau, uint32_t n, int log_n, Xyzz<F>* zs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1u >= n) return;
    Xyzz<F> acc = Xyzz<F>::from_affine(cld(tau + (size_t)n + i));
    Affine<F> b = cld(tau + i);
    if (!b.is_inf()) {
        b.y = -b.y;
        xyzz_madd_inplace(acc, b);
    }
    cst(zs + (__brev(i) >> (32 - log_n)), acc);
}
// K of wire w = bA + aB + C (phase2.go:161-170) into its slot; infinity flags of A and
// B1 by value; keep flags for the three compactions (n_wires + 1 each, the last 0)
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_k_flags(const Xyzz<F>* abc, const Xyzz<F>* ba_ab, uint32_t nw,
                                                      uint32_t nb_public, Xyzz<F>* vk_k, Xyzz<F>* pk_k, uint8_t* inf_a,
                                                      uint8_t* inf_b, uint32_t* keep_a, uint32_t* keep_b) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nw) return;
    if (w == nw) {
        keep_a[w] = 0;
        keep_b[w] = 0;
        return;
    }
    const bool za = cld(abc + w).is_inf(), zb = cld(abc + (size_t)nw + w).is_inf();
    inf_a[w] = za;
    inf_b[w] = zb;
    keep_a[w] = !za;
    keep_b[w] = !zb;
    Xyzz<F> k = cld(ba_ab + w);
    xyzz_add_inplace(k, cld(ba_ab + (size_t)nw + w));
    xyzz_add_inplace(k, cld(abc + 2 * (size_t)nw + w));
    if (w < nb_public) cst(vk_k + w, k);
    else cst(pk_k + (w - nb_public), k);
}
template <class F>
__global__ void __launch_bounds__(256) k_keep(const Xyzz<F>* x, uint32_t nw, uint32_t* keep) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nw) return;
    keep[w] = w < nw && !cld(x + w).is_inf() ? 1u : 0u;
}
template <class F>
__global__ void __launch_bounds__(256) k_compact_pts(const Xyzz<F>* in, const uint32_t* pos, uint32_t nw,
                                                     Xyzz<F>* out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    if (pos[w + 1] != pos[w]) cst(out + pos[w], cld(in + w));
}
// out[i] = k in[i], one scalar for all (canonical, 8 words in HBM)
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_scale(const Affine<F>* in, size_t n, const uint32_t* kcanon,
                                                    Xyzz<F>* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> p = cld(in + i);
    if (p.is_inf()) {
        cst(out + i, Xyzz<F>::inf());
        return;
    }
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = kcanon[j];
    cst(out + i, pt_mul<F>(p, k));
}

// ---------------------------------------------------------------- host
// out[i] = affine(cur[i]), i < n (one inversion per thread of comb.h's kernel)
template <class F>
static void normalize(const Xyzz<F>* cur, size_t n, Affine<F>* out, DevBuf& prefix, hipStream_t st) {
    if (!n) return;
    prefix.reserve(n * sizeof(F));
    const size_t T = std::min<size_t>(n, std::max<size_t>(16384, n / 64));
    hipLaunchKernelGGL(comb::k_comb_normalize<F>, dim3(grid_for(T, 256)), dim3(256), 0, st, cur, n, T, prefix.as<F>(),
                       out);
    GG_HIP(hipGetLastError());
}

// what the three accumulation runs share
struct Ctx {
    hipStream_t st;
    size_t nw;
    const uint32_t* list_off;  // 3 nw + 1
    const uint2* ent;
    const uint8_t* ccls;
    const uint32_t* kcanon;
    const uint32_t* rank;   // nterms + 1
    const uint32_t* glist;  // the general entries in entry order
    uint32_t eb[4], gb[4];  // per side: its first entry, its first general term
    std::vector<std::unique_ptr<DevBuf>>* tmp;
    gg_g16_setup* h;
};
struct Ev {
    hipEvent_t e = nullptr;
    Ev() { GG_HIP(hipEventCreate(&e)); }
    ~Ev() { (void)hipEventDestroy(e); }
};

// out[k - side0 nw] = sum over the list of key k of coefficient * src[side][constraint],
// for the keys of sides [side0, side1); ms[0] the general pass, ms[1] the rounds
template <class F>
static void accumulate(const Ctx& c, uint32_t side0, uint32_t side1, const Affine<F>* const* src, Xyzz<F>* out,
                       double* ms) {
    hipStream_t st = c.st;
    const size_t nk = (size_t)(side1 - side0) * c.nw;
    Src<F> s;
    for (int i = 0; i < 3; i++) s.t[i] = src[i];
    for (int i = 0; i < 4; i++) s.eb[i] = c.eb[i];
    GG_HIP(hipMemsetAsync(out, 0, nk * sizeof(Xyzz<F>), st));
    const uint32_t g0 = c.gb[side0], ng = c.gb[side1] - g0;
    DevBuf gen(std::max<size_t>(ng, 1) * sizeof(Xyzz<F>));
    Ev e0, e1;
    GG_HIP(hipEventRecord(e0.e, st));
    if (ng) {
        hipLaunchKernelGGL(k_gen_mul<F>, dim3(grid_for(ng, PT_BLOCK)), dim3(PT_BLOCK), 0, st, s, c.ent, c.glist, g0, ng,
                           c.kcanon, gen.as<Xyzz<F>>());
        GG_HIP(hipGetLastError());
    }
    GG_HIP(hipEventRecord(e1.e, st));
    GG_WAIT_STREAM(st);
    float gms = 0;
    GG_HIP(hipEventElapsedTime(&gms, e0.e, e1.e));
    AccStats stats;
    acc_rounds<ACC_CHUNK_PTS>(
        c.list_off + (size_t)side0 * c.nw, nk, sizeof(Xyzz<F>), st, *c.tmp, stats,
        [&](bool first, const uint32_t* prev_off, const uint32_t* thr_off, uint32_t nthr, const void* psrc,
            void* pdst) {
            if (first)
                hipLaunchKernelGGL((k_acc_pts<F, true>), dim3(grid_for(nthr, PT_BLOCK)), dim3(PT_BLOCK), 0, st, prev_off,
                                   thr_off, (uint32_t)nk, nthr, (uint32_t)c.nw, side0, c.ent, c.ccls, s, c.rank, g0,
                                   (const Xyzz<F>*)gen.p, (const Xyzz<F>*)nullptr, (Xyzz<F>*)pdst, out);
            else
                hipLaunchKernelGGL((k_acc_pts<F, false>), dim3(grid_for(nthr, PT_BLOCK)), dim3(PT_BLOCK), 0, st,
                                   prev_off, thr_off, (uint32_t)nk, nthr, (uint32_t)c.nw, side0, (const uint2*)nullptr,
                                   (const uint8_t*)nullptr, s, (const uint32_t*)nullptr, g0, (const Xyzz<F>*)nullptr,
                                   (const Xyzz<F>*)psrc, (Xyzz<F>*)pdst, out);
        });
    c.h->acc_launches += stats.launches;
    c.h->ms[6] += stats.kernel_ms;
    c.h->ms[7] += stats.threads;
    ms[0] = gms;
    ms[1] = stats.kernel_ms;
}

struct SrsArgs {
    int curve;
    size_t nw, ncons, nb_public, ncoef, srs_n;
    const uint32_t *off, *wire, *cidx;
    const void* coeffs;
    const void *tau_g1, *alpha_tau_g1, *beta_tau_g1, *tau_g2, *beta_g2;
    int tau_g1_dev, alpha_dev, beta_dev, tau_g2_dev, beta_g2_dev, check_points;
    const void *omega, *g1, *g2;
};

// the device view of `bytes` at p (p itself, or an upload into buf)
static const void* dev_view(const void* p, int on_device, size_t bytes, DevBuf& buf, hipStream_t st) {
    if (on_device) return p;
    upload(buf, p, bytes, st);
    return buf.p;
}

// the point checks over the used prefix of one SRS part: 0 good, 1 off the curve,
// 2 outside the subgroup (the endomorphism tests on BLS12-381)
static void check_part(int curve, bool g2, const void* dev, size_t n, const char* name) {
    std::vector<uint8_t> flags(n);
    int rc;
    if (curve == GG_CURVE_BN254) rc = g2 ? gg_g2_check_bn254(n, dev, flags.data()) : gg_g1_check_bn254(n, dev, flags.data());
    else rc = g2 ? gg_g2_check_endo_bls12_381(n, dev, flags.data()) : gg_g1_check_endo_bls12_381(n, dev, flags.data());
    if (rc != GG_OK) throw Error(rc, std::string("point check of ") + name + ": " + gg_last_error());
    for (size_t i = 0; i < n; i++)
        if (flags[i])
            throw Error(GG_ERR_INVALID_ARG, std::string(name) + "[" + std::to_string(i) + "] is " +
                                                (flags[i] == 1 ? "not on the curve" : "not in the subgroup of order r"));
}
static void refuse_infinity(const void* dev, size_t index, size_t pt, const std::string& name, hipStream_t st) {
    std::vector<uint8_t> p(pt);
    GG_HIP(hipMemcpyAsync(p.data(), (const char*)dev + index * pt, pt, hipMemcpyDeviceToHost, st));
    GG_WAIT_STREAM(st);
    GG_CHECK(std::any_of(p.begin(), p.end(), [](uint8_t b) { return b != 0; }), GG_ERR_INVALID_ARG,
             name + " is the point at infinity");
}

// FC the scalar field; G1F / G2F the coordinate types of the kernels (G2F =
// Called<Fp2Bls> over BLS12-381: the same bytes as Fp2Bls)
template <class FC, class G1F, class G2F>
void run_from_srs(const SrsArgs& a, gg_g16_setup* h) {
    using F = Fe<FC>;
    using A1 = Affine<G1F>;
    using A2 = Affine<G2F>;
    using X1 = Xyzz<G1F>;
    using X2 = Xyzz<G2F>;
    hipStream_t st = hipStreamPerThread;
    Timer tm;
    // ---- host checks (before anything touches the device)
    GG_CHECK(a.ncons >= 1 && a.ncons <= ((size_t)1 << 27), GG_ERR_INVALID_ARG,
             "constraint count out of range (1 .. 2^27)");
    int log_n = 0;
    while (((size_t)1 << log_n) < a.ncons) log_n++;
    const size_t n = (size_t)1 << log_n;
    GG_CHECK(a.srs_n >= 1 && (a.srs_n & (a.srs_n - 1)) == 0, GG_ERR_INVALID_ARG,
             "srs_n " + std::to_string(a.srs_n) + " is not a power of two");
    GG_CHECK(a.srs_n >= n, GG_ERR_INVALID_ARG,
             "srs_n " + std::to_string(a.srs_n) + " is below the domain of n_constraints (" + std::to_string(n) + ")");
    GG_CHECK(a.nw >= 1 && a.nw < 0xffffffffu, GG_ERR_INVALID_ARG, "wire count out of range");
    GG_CHECK(a.nb_public <= a.nw, GG_ERR_INVALID_ARG, "nb_public exceeds n_wires");
    const size_t nrows = 3 * a.ncons;
    const size_t nterms = check_terms(a.nw, a.ncons, a.ncoef, a.off, a.wire, a.cidx);
    const size_t nk = 3 * a.nw;
    F omega;
    memcpy(&omega, a.omega, sizeof(F));
    GG_CHECK(pow2k(omega, log_n) == F::one() && (log_n == 0 || pow2k(omega, log_n - 1) != F::one()),
             GG_ERR_INVALID_ARG, "omega is not a generator of the domain of n_constraints");
    // coefficients by value
    std::vector<uint8_t> ccls(a.ncoef);
    std::vector<uint32_t> kcanon(8 * a.ncoef);
    {
        const F one = F::one(), two = one + one, minus_one = -one;
        for (size_t i = 0; i < a.ncoef; i++) {
            F c;
            memcpy(&c, (const char*)a.coeffs + 32 * i, sizeof(F));
            ccls[i] = c.is_zero() ? C_ZERO : c == one ? C_ONE : c == two ? C_TWO : c == minus_one ? C_MINUS_ONE : C_GENERAL;
            const F k = from_mont(c);
            memcpy(&kcanon[8 * i], k.v, 32);
        }
    }

    GG_HIP(hipGetDevice(&h->device));
    h->curve = a.curve;
    h->from_srs = true;
    h->log_n = log_n;
    h->acc_chunk = ACC_CHUNK_PTS;
    h->nw = a.nw;
    h->g1b = sizeof(A1);
    h->g2b = sizeof(A2);
    h->n_vk = a.nb_public;
    h->nK = a.nw - a.nb_public;
    h->nZ = n - 1;
    h->k_wire_index.resize(h->nK);
    for (size_t i = 0; i < h->nK; i++) h->k_wire_index[i] = (uint32_t)(a.nb_public + i);
    h->ck_base.assign(1, 0);

    std::vector<std::unique_ptr<DevBuf>> tmp;
    auto u32 = [](DevBuf& b) { return b.as<uint32_t>(); };
    auto rd32 = [&](const uint32_t* p) {
        uint32_t v = 0;
        GG_HIP(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
        return v;
    };

    // ---- the SRS in HBM; the point checks
    DevBuf b_tau1, b_alpha, b_beta, b_tau2, b_beta2;
    const size_t ntau = 2 * n - 1;
    const A1* tau1 = (const A1*)dev_view(a.tau_g1, a.tau_g1_dev, ntau * sizeof(A1), b_tau1, st);
    const A1* alpha1 = (const A1*)dev_view(a.alpha_tau_g1, a.alpha_dev, n * sizeof(A1), b_alpha, st);
    const A1* beta1 = (const A1*)dev_view(a.beta_tau_g1, a.beta_dev, n * sizeof(A1), b_beta, st);
    const A2* tau2 = (const A2*)dev_view(a.tau_g2, a.tau_g2_dev, n * sizeof(A2), b_tau2, st);
    const A2* beta2 = (const A2*)dev_view(a.beta_g2, a.beta_g2_dev, sizeof(A2), b_beta2, st);
    GG_WAIT_STREAM(st);
    if (a.check_points) {
        check_part(a.curve, false, tau1, ntau, "tau_g1");
        check_part(a.curve, false, alpha1, n, "alpha_tau_g1");
        check_part(a.curve, false, beta1, n, "beta_tau_g1");
        check_part(a.curve, true, tau2, n, "tau_g2");
        check_part(a.curve, true, beta2, 1, "beta_g2");
        if (n > 1) {
            refuse_infinity(tau1, 1, sizeof(A1), "tau_g1[1]", st);
            refuse_infinity(tau2, 1, sizeof(A2), "tau_g2[1]", st);
        }
        refuse_infinity(alpha1, 0, sizeof(A1), "alpha_tau_g1[0]", st);
        refuse_infinity(beta1, 0, sizeof(A1), "beta_tau_g1[0]", st);
        refuse_infinity(beta2, 0, sizeof(A2), "beta_g2", st);
    }
    h->ms[13] = tm.lap();

    // ---- 2. transposed system
    DevBuf d_off, d_wire, d_cidx, d_ccls, d_kcanon;
    upload(d_off, a.off, (nrows + 1) * 4, st);
    upload(d_wire, a.wire, nterms * 4, st);
    upload(d_cidx, a.cidx, nterms * 4, st);
    upload(d_ccls, ccls.data(), ccls.size(), st);
    upload(d_kcanon, kcanon.data(), kcanon.size() * 4, st);
    DevBuf cnt((nk + 1) * 4), list_off((nk + 1) * 4), cursor(nk * 4), ent(std::max<size_t>(nterms, 1) * 8);
    GG_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes, st));
    GG_HIP(hipMemsetAsync(cursor.p, 0, cursor.bytes, st));
    hipLaunchKernelGGL(k_count, dim3(grid_for(nrows, 256)), dim3(256), 0, st, u32(d_off), u32(d_wire),
                       (uint32_t)nrows, (uint32_t)a.nw, u32(cnt));
    GG_HIP(hipGetLastError());
    uscan(u32(cnt), u32(list_off), nk + 1, st, tmp);
    hipLaunchKernelGGL(k_fill, dim3(grid_for(nrows, 256)), dim3(256), 0, st, u32(d_off), u32(d_wire), u32(d_cidx),
                       (uint32_t)nrows, (uint32_t)a.nw, u32(list_off), u32(cursor), ent.as<uint2>());
    GG_HIP(hipGetLastError());
    // ---- 3. the general terms, numbered in entry order
    DevBuf rank((nterms + 1) * 4);
    hipLaunchKernelGGL(k_gen_flag, dim3(grid_for(nterms + 1, 256)), dim3(256), 0, st, (const uint2*)ent.p,
                       (const uint8_t*)d_ccls.p, (uint32_t)nterms, u32(rank));
    GG_HIP(hipGetLastError());
    uscan(u32(rank), u32(rank), nterms + 1, st, tmp);
    Ctx c;
    c.st = st;
    c.nw = a.nw;
    c.list_off = u32(list_off);
    c.ent = ent.as<uint2>();
    c.ccls = d_ccls.as<uint8_t>();
    c.kcanon = u32(d_kcanon);
    c.rank = u32(rank);
    c.tmp = &tmp;
    c.h = h;
    for (int s = 0; s < 4; s++) {
        c.eb[s] = rd32(u32(list_off) + (size_t)s * a.nw);
        c.gb[s] = rd32(u32(rank) + c.eb[s]);
    }
    const uint32_t ngen = c.gb[3];
    DevBuf glist(std::max<size_t>(ngen, 1) * 4);
    if (nterms) {
        hipLaunchKernelGGL(k_gen_list, dim3(grid_for(nterms, 256)), dim3(256), 0, st, (const uint32_t*)rank.p,
                           (uint32_t)nterms, u32(glist));
        GG_HIP(hipGetLastError());
    }
    c.glist = u32(glist);
    GG_WAIT_STREAM(st);
    cursor.release();
    cnt.release();
    d_wire.release();
    d_cidx.release();
    h->ms[0] = tm.lap();
    h->ms[8] = (double)nterms;
    h->ms[23] = (double)ngen;

    // ---- 1. Lagrange forms (the Lagrange form of one point is the point)
    DevBuf l1(n * sizeof(A1)), la(n * sizeof(A1)), lb(n * sizeof(A1)), l2(n * sizeof(A2));
    {
        Timer te;
        auto lag = [&](bool g2, const void* in, DevBuf& out, int slot) {
            if (log_n == 0) {
                GG_HIP(hipMemcpyAsync(out.p, in, out.bytes, hipMemcpyDeviceToDevice, st));
                GG_WAIT_STREAM(st);
            } else if (g2) {
                ecntt::to_lagrange_g2_dev(a.curve, log_n, a.omega, in, out.p, st, nullptr);
            } else {
                ecntt::to_lagrange_dev(a.curve, log_n, a.omega, in, out.p, st, nullptr);
            }
            h->ms[slot] = te.lap();
        };
        lag(false, tau1, l1, 9);
        lag(false, alpha1, la, 10);
        lag(false, beta1, lb, 11);
        lag(true, tau2, l2, 12);
    }
    h->ms[1] = tm.lap();

    // ---- 4. accumulate
    DevBuf abc(nk * sizeof(X1)), ba_ab(2 * a.nw * sizeof(X1)), b2(a.nw * sizeof(X2));
    {
        const A1* s1[3] = {l1.as<A1>(), l1.as<A1>(), l1.as<A1>()};
        accumulate<G1F>(c, 0, 3, s1, abc.as<X1>(), &h->ms[14]);
        const A1* s2[3] = {lb.as<A1>(), la.as<A1>(), nullptr};
        accumulate<G1F>(c, 0, 2, s2, ba_ab.as<X1>(), &h->ms[16]);
        const A2* s3[3] = {nullptr, l2.as<A2>(), nullptr};
        accumulate<G2F>(c, 1, 2, s3, b2.as<X2>(), &h->ms[18]);
    }
    l1.release();
    la.release();
    lb.release();
    l2.release();
    ent.release();
    rank.release();
    glist.release();
    h->ms[2] = tm.lap();

    // ---- 5. K, Z, flags, compaction (XYZZ)
    const size_t nvk = h->n_vk, npk = h->nK;
    DevBuf x_vk(std::max<size_t>(nvk, 1) * sizeof(X1)), x_pk(std::max<size_t>(npk, 1) * sizeof(X1));
    DevBuf keep_a((a.nw + 1) * 4), keep_b((a.nw + 1) * 4), keep_b2((a.nw + 1) * 4);
    h->inf_a.alloc(a.nw);
    h->inf_b.alloc(a.nw);
    hipLaunchKernelGGL(k_k_flags<G1F>, dim3(grid_for(a.nw + 1, PT_BLOCK)), dim3(PT_BLOCK), 0, st,
                       (const X1*)abc.p, (const X1*)ba_ab.p, (uint32_t)a.nw, (uint32_t)a.nb_public, x_vk.as<X1>(),
                       x_pk.as<X1>(), h->inf_a.as<uint8_t>(), h->inf_b.as<uint8_t>(), u32(keep_a), u32(keep_b));
    GG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_keep<G2F>, dim3(grid_for(a.nw + 1, 256)), dim3(256), 0, st, (const X2*)b2.p,
                       (uint32_t)a.nw, u32(keep_b2));
    GG_HIP(hipGetLastError());
    uscan(u32(keep_a), u32(keep_a), a.nw + 1, st, tmp);
    uscan(u32(keep_b), u32(keep_b), a.nw + 1, st, tmp);
    uscan(u32(keep_b2), u32(keep_b2), a.nw + 1, st, tmp);
    h->nA = rd32(u32(keep_a) + a.nw);
    h->nB = rd32(u32(keep_b) + a.nw);
    const size_t nB2 = rd32(u32(keep_b2) + a.nw);
    GG_CHECK(nB2 == h->nB, GG_ERR_INVALID_ARG,
             "tau_g1 and tau_g2 disagree: " + std::to_string(h->nB) + " B wires are not the infinity in G1, " +
                 std::to_string(nB2) + " in G2");
    DevBuf x_a(std::max<size_t>(h->nA, 1) * sizeof(X1)), x_b(std::max<size_t>(h->nB, 1) * sizeof(X1));
    DevBuf x_b2(std::max<size_t>(h->nB, 1) * sizeof(X2)), x_z(std::max<size_t>(h->nZ, 1) * sizeof(X1));
    hipLaunchKernelGGL(k_compact_pts<G1F>, dim3(grid_for(a.nw, 256)), dim3(256), 0, st, (const X1*)abc.p,
                       (const uint32_t*)keep_a.p, (uint32_t)a.nw, x_a.as<X1>());
    GG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_compact_pts<G1F>, dim3(grid_for(a.nw, 256)), dim3(256), 0, st, (const X1*)abc.p + a.nw,
                       (const uint32_t*)keep_b.p, (uint32_t)a.nw, x_b.as<X1>());
    GG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_compact_pts<G2F>, dim3(grid_for(a.nw, 256)), dim3(256), 0, st, (const X2*)b2.p,
                       (const uint32_t*)keep_b2.p, (uint32_t)a.nw, x_b2.as<X2>());
    GG_HIP(hipGetLastError());
    GG_WAIT_STREAM(st);
    const double kms = tm.lap();
    if (h->nZ) {
        hipLaunchKernelGGL(k_z<G1F>, dim3(grid_for(n, PT_BLOCK)), dim3(PT_BLOCK), 0, st, tau1, (uint32_t)n, log_n,
                           x_z.as<X1>());
        GG_HIP(hipGetLastError());
        GG_WAIT_STREAM(st);
    }
    h->ms[20] = tm.lap();
    h->ms[3] = kms + h->ms[20];
    abc.release();
    ba_ab.release();
    b2.release();

    // ---- normalise: one batch inversion per output array (the scratch at its
    // largest size first: no buffer is replaced between the launches)
    DevBuf prefix;
    prefix.reserve(std::max({(size_t)1, h->nA, h->nB, h->nZ, nvk, npk}) * sizeof(G1F));
    auto out1 = [&](DevBuf& x, size_t cnt_, DevBuf& out) {
        out.alloc(std::max<size_t>(cnt_, 1) * sizeof(A1));
        normalize<G1F>((const X1*)x.p, cnt_, out.as<A1>(), prefix, st);
    };
    out1(x_a, h->nA, h->g1_A);
    out1(x_b, h->nB, h->g1_B);
    out1(x_z, h->nZ, h->g1_Z);
    out1(x_vk, nvk, h->vk_K);
    out1(x_pk, npk, h->g1_K);
    h->g1_abd.alloc(3 * sizeof(A1));  // alpha, beta (setup.go:30-31), delta = the generator (phase2.go:143)
    GG_HIP(hipMemcpyAsync(h->g1_abd.p, alpha1, sizeof(A1), hipMemcpyDeviceToDevice, st));
    GG_HIP(hipMemcpyAsync((char*)h->g1_abd.p + sizeof(A1), beta1, sizeof(A1), hipMemcpyDeviceToDevice, st));
    GG_HIP(hipMemcpyAsync((char*)h->g1_abd.p + 2 * sizeof(A1), a.g1, sizeof(A1), hipMemcpyHostToDevice, st));
    GG_WAIT_STREAM(st);
    h->ms[4] = tm.lap();
    h->g2_B.alloc(std::max<size_t>(h->nB, 1) * sizeof(A2));
    normalize<G2F>((const X2*)x_b2.p, h->nB, h->g2_B.as<A2>(), prefix, st);
    h->g2_tail.alloc(5 * sizeof(A2));  // beta (setup.go:37), delta and gamma = the generator (phase2.go:144, setup.go:88)
    GG_HIP(hipMemsetAsync(h->g2_tail.p, 0, h->g2_tail.bytes, st));
    GG_HIP(hipMemcpyAsync(h->g2_tail.p, beta2, sizeof(A2), hipMemcpyDeviceToDevice, st));
    GG_HIP(hipMemcpyAsync((char*)h->g2_tail.p + sizeof(A2), a.g2, sizeof(A2), hipMemcpyHostToDevice, st));
    GG_HIP(hipMemcpyAsync((char*)h->g2_tail.p + 2 * sizeof(A2), a.g2, sizeof(A2), hipMemcpyHostToDevice, st));
    GG_WAIT_STREAM(st);
    h->ms[5] = tm.lap();
    h->ms[21] = h->ms[4] + h->ms[5];
}

// p[i] *= k in place (affine), i < n
template <class F>
static void scale(DevBuf& pts, size_t off, size_t n, const uint32_t* kcanon_dev, DevBuf& cur, DevBuf& prefix,
                  hipStream_t st) {
    if (!n) return;
    cur.reserve(n * sizeof(Xyzz<F>));
    Affine<F>* p = (Affine<F>*)((char*)pts.p + off);
    hipLaunchKernelGGL(k_scale<F>, dim3(grid_for(n, PT_BLOCK)), dim3(PT_BLOCK), 0, st, (const Affine<F>*)p, n, kcanon_dev,
                       cur.as<Xyzz<F>>());
    GG_HIP(hipGetLastError());
    normalize<F>((const Xyzz<F>*)cur.p, n, p, prefix, st);
}

template <class FC, class G1F, class G2F>
void run_contribute(gg_g16_setup* h, const void* delta_mont) {
    using F = Fe<FC>;
    F delta;
    memcpy(&delta, delta_mont, sizeof(F));
    Timer tm;
    hipStream_t st = hipStreamPerThread;
    int dev = 0;
    GG_HIP(hipGetDevice(&dev));
    GG_CHECK(dev == h->device, GG_ERR_INVALID_ARG,
             "the key lives on device " + std::to_string(h->device) + ", the calling thread is on device " +
                 std::to_string(dev));
    const F ks[2] = {from_mont(delta), from_mont(inverse(delta))};
    WipeBuf d_k(sizeof(ks));
    GG_HIP(hipMemcpyAsync(d_k.p, ks, sizeof(ks), hipMemcpyHostToDevice, st));
    const uint32_t* kd = d_k.as<uint32_t>();
    DevBuf cur, prefix;
    const size_t mx = std::max({(size_t)1, h->nZ, h->nK});  // no buffer is replaced between the launches
    cur.reserve(mx * sizeof(Xyzz<G1F>));
    prefix.reserve(mx * sizeof(G1F));
    scale<G1F>(h->g1_abd, 2 * sizeof(Affine<G1F>), 1, kd, cur, prefix, st);  // phase2.go:195
    scale<G1F>(h->g1_Z, 0, h->nZ, kd + 8, cur, prefix, st);                  // phase2.go:199-201
    scale<G1F>(h->g1_K, 0, h->nK, kd + 8, cur, prefix, st);                  // phase2.go:204-206
    GG_WAIT_STREAM(st);
    cur.release();
    prefix.release();
    scale<G2F>(h->g2_tail, sizeof(Affine<G2F>), 1, kd, cur, prefix, st);  // phase2.go:196
    GG_WAIT_STREAM(st);
    h->ms[22] = tm.lap();
}

}  // namespace g16m
}  // namespace gg

using namespace gg;
using namespace gg::g16m;

extern "C" int gg_groth16_setup_from_srs(int curve, size_t n_wires, size_t n_constraints, size_t nb_public,
                                         const uint32_t* term_off, const uint32_t* term_wire,
                                         const uint32_t* term_coeff, const void* coeffs, size_t n_coeffs,
                                         const void* tau_g1, int tau_g1_on_device, const void* alpha_tau_g1,
                                         int alpha_tau_g1_on_device, const void* beta_tau_g1,
                                         int beta_tau_g1_on_device, const void* tau_g2, int tau_g2_on_device,
                                         const void* beta_g2, int beta_g2_on_device, size_t srs_n, int check_points,
                                         const void* omega_mont, const void* g1_gen, const void* g2_gen,
                                         gg_g16_setup_t* out) {
    GG_CAPI_BEGIN
    const char* null_arg = !out            ? "out"
                           : !term_off     ? "term_off"
                           : !coeffs       ? "coeffs"
                           : !tau_g1       ? "tau_g1"
                           : !alpha_tau_g1 ? "alpha_tau_g1"
                           : !beta_tau_g1  ? "beta_tau_g1"
                           : !tau_g2       ? "tau_g2"
                           : !beta_g2      ? "beta_g2"
                           : !omega_mont   ? "omega_mont"
                           : !g1_gen       ? "g1_gen"
                           : !g2_gen       ? "g2_gen"
                                           : nullptr;
    GG_CHECK(!null_arg, GG_ERR_INVALID_ARG, std::string("null argument: ") + (null_arg ? null_arg : ""));
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG, "unknown curve");
    const SrsArgs a{curve,       n_wires,          n_constraints,          nb_public,
                    n_coeffs,    srs_n,            term_off,               term_wire,
                    term_coeff,  coeffs,           tau_g1,                 alpha_tau_g1,
                    beta_tau_g1, tau_g2,           beta_g2,                tau_g1_on_device,
                    alpha_tau_g1_on_device,        beta_tau_g1_on_device,  tau_g2_on_device,
                    beta_g2_on_device,             check_points,           omega_mont,
                    g1_gen,      g2_gen};
    std::unique_ptr<gg_g16_setup> h(new gg_g16_setup());
    if (curve == GG_CURVE_BN254) run_from_srs<FrCfg, Fp, Fp2>(a, h.get());
    else run_from_srs<FrBlsCfg, FpBls, G2Bls>(a, h.get());
    *out = h.release();
    GG_CAPI_END
}

extern "C" int gg_groth16_setup_contribute(gg_g16_setup_t h, const void* delta) {
    GG_CAPI_BEGIN
    GG_CHECK(delta, GG_ERR_INVALID_ARG, "null argument: delta");
    {  // zero has one encoding on both curves: refused before the handle is looked at
        const uint8_t* d = (const uint8_t*)delta;
        GG_CHECK(std::any_of(d, d + 32, [](uint8_t b) { return b != 0; }), GG_ERR_INVALID_ARG, "delta is zero");
    }
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    GG_CHECK(h->from_srs, GG_ERR_INVALID_ARG,
             "this key was made by gg_groth16_setup from the toxic waste: only a key from gg_groth16_setup_from_srs "
             "takes contributions");
    if (h->curve == GG_CURVE_BN254) run_contribute<FrCfg, Fp, Fp2>(h, delta);
    else run_contribute<FrBlsCfg, FpBls, G2Bls>(h, delta);
    GG_CAPI_END
}

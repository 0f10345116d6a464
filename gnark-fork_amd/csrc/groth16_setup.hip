// Groth16 Setup on the GPU (backend/groth16/bn254/setup.go:85-337 and the same
// file under bls12-381/): from the R1CS matrices (the CSR of gg_r1cs_create_ex)
// and the toxic waste to the points of gnark's ProvingKey / VerifyingKey.
// Templated over the scalar field as the solver is.  All intermediate scalars
// stay in HBM; nothing goes back to the host before gg_groth16_setup_read except
// a few counts (list totals, nA, nB).
//
//   1. Lagrange table  L_j(tau) = (tau^n - 1)/n * w^j / (tau - w^j), j < n_constraints:
//      the closed form of the recurrence of setup.go:376-428 (the same field
//      element), w^j by plk::scan_prod, the denominators by plk::batch_invert.
//   2. Transposed system: per key (side, wire) the list of its (constraint,
//      coefficient id) pairs -- count, scan, fill.  The order inside a list is
//      whatever the fill's atomics give: field addition is exact (associative
//      and commutative, no rounding), so the sum does not depend on it.
//   3. Accumulate (setupABC, setup.go:411-430): A[w], B[w], C[w] = sum coeff * L_j
//      over the key's list.  Lists are badly skewed (the ONE wire carries a term
//      in a third of all constraints, most wires carry three), so no thread walks
//      a list: every list is cut into chunks of ACC_CHUNK entries, one thread
//      per chunk writes a partial sum, and the partials of the keys that still
//      have more than one are cut again -- ceil(log_ACC_CHUNK(max degree))
//      rounds, each one launch (plus the scan that numbers its chunks), whatever
//      the degree.  A thread finds its key by binary search in the scanned
//      chunk offsets.  Every coefficient id is a product with the table (ids 0
//      to 3 hold 0, 1, 2, -1: no special cases).
//   4. K per wire, scattered to its class slot (gg_groth16_setup_layout); Z
//      bit-reversed as scalars; infinity flags by value; A and B compacted.
//   5. Points: the 8-bit comb of batch.hip, restated in comb.h so that one table per
//      generator serves every part.
//
// Every device buffer that holds toxic waste or discrete logs is a WipeBuf:
// overwritten with zeros before its memory is freed, on the error paths too.
#include "common.h"
#include "field.cuh"
#include "curve.cuh"
#include "comb.h"
#include "groth16_setup_common.h"
#include "plonk_ops.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gg {
namespace g16s {

// ---- the accumulation's constants (DESIGN.md "Groth16 Setup")
// ACC_CHUNK entries per thread: an entry is 8 B read in sequence plus one 32-B
// gather of L_j and one product (64 VGPRs, no LDS, 8 waves per SIMD as compiled:
// occupancy is not the limit, the gathers are).  32 keeps the ONE wire of a 2^24 MiMC system
// (5.6 M terms) at 5 rounds while the common 1..3-term wires cost one thread.
constexpr uint32_t ACC_CHUNK = 32;

// thread i of nthr: the key whose [thr_off[k], thr_off[k + 1]) holds i, its
// chunk c = i - thr_off[k]; adds at most ACC_CHUNK items.  A key with one thread
// writes its final sum to out[key], the others partial i (so thr_off is also
// the next round's source offsets).
template <class F, bool FIRST>
__global__ void __launch_bounds__(ACC_BLOCK) k_acc(const uint32_t* prev_off, const uint32_t* thr_off, uint32_t nk,
                                                   uint32_t nthr, const uint2* ent, const F* L, const F* coef,
                                                   const F* psrc, F* pdst, F* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthr) return;
    // the last k with thr_off[k] <= i (keys without work share their successor's offset)
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
    const uint32_t b0 = c * ACC_CHUNK;
    const uint32_t m = min(ACC_CHUNK, cnt - b0);
    const size_t base = (size_t)prev_off[k] + b0;
    F acc = F::zero();
    for (uint32_t e = 0; e < m; e++) {
        if (FIRST) {
            const uint2 en = ent[base + e];
            acc = acc + ld_fr(coef + en.y) * ld_fr(L + en.x);
        } else {
            acc = acc + ld_fr(psrc + base + e);
        }
    }
    if (work == 1u) st_fr(out + k, acc);
    else st_fr(pdst + i, acc);
}

// ---------------------------------------------------------------- scalars
template <class F>
__global__ void __launch_bounds__(256) k_fill_geo(F* x, size_t n, F first, F ratio) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_fr(x + i, i ? ratio : first);
}
// den[j] = tau - w^j
template <class F>
__global__ void __launch_bounds__(256) k_den(const F* wj, F* den, size_t n, F tau) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) st_fr(den + j, tau - ld_fr(wj + j));
}
// L[j] = c * w^j / (tau - w^j), in place over the inverted denominators
template <class F>
__global__ void __launch_bounds__(256) k_lagrange(const F* wj, F* L, size_t n, F c) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) st_fr(L + j, c * ld_fr(wj + j) * ld_fr(L + j));
}
// pk.G1.Z scalars: zs[r] = z[brev(r)] for r < n - 1 (setup.go:265-267 on scalars)
template <class F>
__global__ void __launch_bounds__(256) k_z_brev(const F* z, F* zs, uint32_t n, int log_n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = log_n ? (__brev(i) >> (32 - log_n)) : 0u;
    if (r + 1u < n) st_fr(zs + r, ld_fr(z + i));
}
// K of wire w into its class slot; infinity flags by value; keep flags for the compaction
template <class F>
struct KParams {
    const F* abc;  // A | B | C, n_wires each
    const uint32_t* cls;
    const uint32_t* slot;  // slot inside the class (commitment bases: inside the concatenated bases)
    F *vk_k, *pk_k, *ck_k, *ck_sigma;
    uint8_t *inf_a, *inf_b;
    uint32_t *keep_a, *keep_b;  // n_wires + 1 (the last one 0)
    F alpha, beta, gamma_inv, delta_inv, sigma;
    uint32_t nw;
};
template <class F>
__global__ void __launch_bounds__(256) k_key_scalars(KParams<F> P) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > P.nw) return;
    if (w == P.nw) {
        P.keep_a[w] = 0;
        P.keep_b[w] = 0;
        return;
    }
    const F a = ld_fr(P.abc + w), b = ld_fr(P.abc + (size_t)P.nw + w), c = ld_fr(P.abc + 2 * (size_t)P.nw + w);
    const bool za = a.is_zero(), zb = b.is_zero();
    P.inf_a[w] = za;
    P.inf_b[w] = zb;
    P.keep_a[w] = !za;
    P.keep_b[w] = !zb;
    const F t = P.beta * a + P.alpha * b + c;
    const uint32_t cl = P.cls[w], s = P.slot[w];
    if (cl == GG_SETUP_CLASS_PK_K) {
        st_fr(P.pk_k + s, t * P.delta_inv);
    } else {
        const F k = t * P.gamma_inv;
        if (cl == GG_SETUP_CLASS_VK_K) {
            st_fr(P.vk_k + s, k);
        } else {
            st_fr(P.ck_k + s, k);
            st_fr(P.ck_sigma + s, k * P.sigma);
        }
    }
}
template <class F>
__global__ void __launch_bounds__(256) k_compact(const F* in, const uint32_t* pos, uint32_t nw, F* out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    if (pos[w + 1] != pos[w]) st_fr(out + pos[w], ld_fr(in + w));
}

// ---------------------------------------------------------------- host
struct Layout {
    std::vector<uint32_t> cls, slot;
    size_t n_vk = 0, n_pk = 0;
    std::vector<size_t> n_ck;
};

// the loop of setup.go:159-196
static void layout(size_t nw, size_t nb_public, const uint32_t* cw, size_t nc, const uint32_t* coff,
                   const uint32_t* cwire, Layout& L) {
    GG_CHECK(nw >= 1 && nw < 0xffffffffu, GG_ERR_INVALID_ARG, "wire count out of range");
    GG_CHECK(nb_public <= nw, GG_ERR_INVALID_ARG, "nb_public exceeds n_wires");
    GG_CHECK(nc == 0 || (cw && coff), GG_ERR_INVALID_ARG, "null commitment arrays");
    GG_CHECK(nc < 0x7fffffffu, GG_ERR_INVALID_ARG, "too many commitments");
    if (nc) {
        GG_CHECK(coff[0] == 0, GG_ERR_INVALID_ARG, "committed_off[0] must be 0");
        for (size_t j = 0; j < nc; j++)
            GG_CHECK(coff[j] <= coff[j + 1], GG_ERR_INVALID_ARG, "committed_off not monotonic");
        GG_CHECK(coff[nc] == 0 || cwire, GG_ERR_INVALID_ARG, "null committed_wire");
    }
    auto range_check = [&](uint32_t w, const std::string& what) {
        GG_CHECK(w >= nb_public, GG_ERR_INVALID_ARG, what + " wire " + std::to_string(w) + " is below nb_public (a public wire)");
        GG_CHECK(w < nw, GG_ERR_INVALID_ARG, what + " wire " + std::to_string(w) + " is not below n_wires");
    };
    constexpr uint32_t NONE = 0xffffffffu;
    L.cls.assign(nw, GG_SETUP_CLASS_PK_K);
    L.slot.assign(nw, 0);
    L.n_ck.assign(nc, 0);
    std::vector<uint32_t> owner(nw, NONE);
    for (size_t j = 0; j < nc; j++) {
        range_check(cw[j], "commitment");
        GG_CHECK(j == 0 || cw[j - 1] < cw[j], GG_ERR_INVALID_ARG,
                 "commitment wires not strictly increasing at wire " + std::to_string(cw[j]));
        L.cls[cw[j]] = GG_SETUP_CLASS_VK_K;
    }
    for (size_t j = 0; j < nc; j++)
        for (uint32_t t = coff[j]; t < coff[j + 1]; t++) {
            const uint32_t w = cwire[t];
            range_check(w, "committed");
            GG_CHECK(t == coff[j] || cwire[t - 1] < w, GG_ERR_INVALID_ARG,
                     "committed wires of commitment " + std::to_string(j) + " not strictly increasing at wire " +
                         std::to_string(w));
            GG_CHECK(owner[w] == NONE, GG_ERR_INVALID_ARG,
                     "wire " + std::to_string(w) + " is committed by two commitments");
            GG_CHECK(L.cls[w] != GG_SETUP_CLASS_VK_K, GG_ERR_INVALID_ARG,
                     "wire " + std::to_string(w) + " is a commitment wire and privately committed");
            owner[w] = (uint32_t)j;
            L.cls[w] = GG_SETUP_CLASS_CK + (uint32_t)j;
        }
    for (size_t i = 0; i < nb_public; i++) L.cls[i] = GG_SETUP_CLASS_VK_K;
    // slots in wire order: vI, cI[j] and i - vI - nbPrivateCommittedSeen of the reference
    for (size_t i = 0; i < nw; i++) {
        const uint32_t c = L.cls[i];
        if (c == GG_SETUP_CLASS_VK_K) L.slot[i] = (uint32_t)L.n_vk++;
        else if (c == GG_SETUP_CLASS_PK_K) L.slot[i] = (uint32_t)L.n_pk++;
        else L.slot[i] = (uint32_t)L.n_ck[c - GG_SETUP_CLASS_CK]++;
    }
}


}  // namespace g16s
}  // namespace gg

using namespace gg;
using namespace gg::g16s;
using gg::comb::CombScratch;
using gg::comb::CombTable;
using gg::comb::comb_mul;


namespace {

struct SetupArgs {
    size_t nw, ncons, nb_public, ncoef, ncommit;
    const uint32_t *off, *wire, *cidx, *cw, *coff, *cwire;
    const void *coeffs, *tau, *alpha, *beta, *gamma, *delta, *sigma, *pg, *omega, *g1, *g2;
};

template <class FC, class G1F, class G2F>
void run_setup(const SetupArgs& a, gg_g16_setup* h) {
    using F = Fe<FC>;
    hipStream_t st = hipStreamPerThread;
    Timer tm;
    // ---- host checks (before anything touches the device)
    GG_CHECK(a.ncons >= 1 && a.ncons <= ((size_t)1 << 28), GG_ERR_INVALID_ARG,
             "constraint count out of range (1 .. 2^28)");
    int log_n = 0;
    while (((size_t)1 << log_n) < a.ncons) log_n++;
    const size_t n = (size_t)1 << log_n;
    Layout lay;
    layout(a.nw, a.nb_public, a.cw, a.ncommit, a.coff, a.cwire, lay);
    const size_t nrows = 3 * a.ncons;
    const size_t nterms = check_terms(a.nw, a.ncons, a.ncoef, a.off, a.wire, a.cidx);
    const size_t nk = 3 * a.nw;
    auto fe = [](const void* p) {
        F x;
        memcpy(&x, p, sizeof(F));
        return x;
    };
    const F tau = fe(a.tau), alpha = fe(a.alpha), beta = fe(a.beta), gamma = fe(a.gamma), delta = fe(a.delta);
    const F omega = fe(a.omega);
    GG_CHECK(!alpha.is_zero(), GG_ERR_INVALID_ARG, "toxic waste: alpha is zero");
    GG_CHECK(!beta.is_zero(), GG_ERR_INVALID_ARG, "toxic waste: beta is zero");
    GG_CHECK(!gamma.is_zero(), GG_ERR_INVALID_ARG, "toxic waste: gamma is zero");
    GG_CHECK(!delta.is_zero(), GG_ERR_INVALID_ARG, "toxic waste: delta is zero");
    F sigma = F::one(), pg = F::one();
    if (a.ncommit) {
        GG_CHECK(a.sigma && a.pg, GG_ERR_INVALID_ARG, "commitments need pedersen_sigma and pedersen_g");
        sigma = fe(a.sigma);
        pg = fe(a.pg);
        GG_CHECK(!sigma.is_zero(), GG_ERR_INVALID_ARG, "pedersen: sigma is zero");
        GG_CHECK(!pg.is_zero(), GG_ERR_INVALID_ARG, "pedersen: g is zero (G would be the point at infinity)");
    }
    GG_CHECK(pow2k(omega, log_n) == F::one() && (log_n == 0 || pow2k(omega, log_n - 1) != F::one()),
             GG_ERR_INVALID_ARG, "omega is not a generator of the domain of n_constraints");
    const F tn1 = pow2k(tau, log_n) - F::one();  // tau^n - 1
    GG_CHECK(!tn1.is_zero(), GG_ERR_INVALID_ARG,
             "toxic waste: tau^n == 1, tau is in the domain (the reference divides by zero there, setup.go:368-371)");
    F nf = F::zero();
    nf.v[0] = (uint32_t)n;  // n <= 2^28
    const F lag_c = tn1 * inverse(to_mont(nf));
    const F gamma_inv = inverse(gamma), delta_inv = inverse(delta);
    const F zdt = tn1 * delta_inv;

    GG_HIP(hipGetDevice(&h->device));
    h->curve = std::is_same<FC, FrCfg>::value ? GG_CURVE_BN254 : GG_CURVE_BLS12_381;
    h->log_n = log_n;
    h->acc_chunk = ACC_CHUNK;
    h->nw = a.nw;
    h->g1b = sizeof(Affine<G1F>);
    h->g2b = sizeof(Affine<G2F>);
    h->n_vk = lay.n_vk;
    h->nK = lay.n_pk;
    h->nZ = n - 1;
    h->n_ck = lay.n_ck;
    h->ck_base.assign(a.ncommit + 1, 0);
    for (size_t j = 0; j < a.ncommit; j++) h->ck_base[j + 1] = h->ck_base[j] + lay.n_ck[j];
    const size_t n_ck_all = h->ck_base[a.ncommit];
    h->k_wire_index.reserve(lay.n_pk);
    for (size_t i = 0; i < a.nw; i++) {
        if (lay.cls[i] == GG_SETUP_CLASS_PK_K) h->k_wire_index.push_back((uint32_t)i);
        else if (lay.cls[i] >= GG_SETUP_CLASS_CK) lay.slot[i] += (uint32_t)h->ck_base[lay.cls[i] - GG_SETUP_CLASS_CK];
    }

    std::vector<std::unique_ptr<DevBuf>> tmp;  // scan scratch (counts only)
    auto zero = [&](DevBuf& b) { GG_HIP(hipMemsetAsync(b.p, 0, b.bytes, st)); };
    auto u32 = [](DevBuf& b) { return b.as<uint32_t>(); };
    auto rd32 = [&](const uint32_t* p) {
        uint32_t v = 0;
        GG_HIP(hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, st));
        GG_WAIT_STREAM(st);
        return v;
    };

    // ---- 2. transposed system
    DevBuf d_off, d_wire, d_cidx, d_coef, d_cls, d_slot;
    upload(d_off, a.off, (nrows + 1) * 4, st);
    upload(d_wire, a.wire, nterms * 4, st);
    upload(d_cidx, a.cidx, nterms * 4, st);
    upload(d_coef, a.coeffs, a.ncoef * 32, st);
    upload(d_cls, lay.cls.data(), a.nw * 4, st);
    upload(d_slot, lay.slot.data(), a.nw * 4, st);
    DevBuf cnt((nk + 1) * 4), list_off((nk + 1) * 4), cursor(nk * 4), ent(std::max<size_t>(nterms, 1) * 8);
    zero(cnt);
    zero(cursor);
    hipLaunchKernelGGL(k_count, dim3(grid_for(nrows, 256)), dim3(256), 0, st, u32(d_off), u32(d_wire),
                       (uint32_t)nrows, (uint32_t)a.nw, u32(cnt));
    GG_HIP(hipGetLastError());
    uscan(u32(cnt), u32(list_off), nk + 1, st, tmp);
    hipLaunchKernelGGL(k_fill, dim3(grid_for(nrows, 256)), dim3(256), 0, st, u32(d_off), u32(d_wire), u32(d_cidx),
                       (uint32_t)nrows, (uint32_t)a.nw, u32(list_off), u32(cursor), ent.as<uint2>());
    GG_HIP(hipGetLastError());
    GG_WAIT_STREAM(st);
    cursor.release();
    d_wire.release();
    d_cidx.release();
    h->ms[0] = tm.lap();

    // ---- 1. Lagrange table
    Arena ar;
    struct ArenaWipe {  // scan / inversion scratch holds products of (tau - w^j)
        Arena& a;
        ~ArenaWipe() {
            if (a.buf.p) {
                (void)hipMemsetAsync(a.buf.p, 0, a.buf.bytes, hipStreamPerThread);
                (void)hipStreamSynchronize(hipStreamPerThread);
            }
        }
    } arena_wipe{ar};
    ar.reserve(plk::scan_arena_bytes(n) + plk::batch_invert_arena_bytes(n) + 4096);
    WipeBuf Ltab(a.ncons * 32);
    {
        DevBuf wj(a.ncons * 32);  // w^j: public
        hipLaunchKernelGGL(k_fill_geo<F>, dim3(grid_for(a.ncons, 256)), dim3(256), 0, st, wj.as<F>(), a.ncons,
                           F::one(), omega);
        GG_HIP(hipGetLastError());
        plk::scan_prod(wj.as<F>(), a.ncons, st, ar);
        hipLaunchKernelGGL(k_den<F>, dim3(grid_for(a.ncons, 256)), dim3(256), 0, st, (const F*)wj.p, Ltab.as<F>(),
                           a.ncons, tau);
        GG_HIP(hipGetLastError());
        plk::batch_invert(Ltab.as<F>(), a.ncons, st, ar);
        hipLaunchKernelGGL(k_lagrange<F>, dim3(grid_for(a.ncons, 256)), dim3(256), 0, st, (const F*)wj.p,
                           Ltab.as<F>(), a.ncons, lag_c);
        GG_HIP(hipGetLastError());
        GG_WAIT_STREAM(st);
    }
    h->ms[1] = tm.lap();

    // ---- 3. accumulate
    WipeBuf abc(nk * 32);
    zero(abc);
    {
        AccStats stats;
        acc_rounds<ACC_CHUNK>(
            u32(list_off), nk, 32, st, tmp, stats,
            [&](bool first, const uint32_t* prev_off, const uint32_t* thr_off, uint32_t nthr, const void* psrc,
                void* pdst) {
                if (first)
                    hipLaunchKernelGGL((k_acc<F, true>), dim3(grid_for(nthr, ACC_BLOCK)), dim3(ACC_BLOCK), 0, st, prev_off,
                                       thr_off, (uint32_t)nk, nthr, (const uint2*)ent.p, (const F*)Ltab.p,
                                       (const F*)d_coef.p, (const F*)nullptr, (F*)pdst, abc.as<F>());
                else
                    hipLaunchKernelGGL((k_acc<F, false>), dim3(grid_for(nthr, ACC_BLOCK)), dim3(ACC_BLOCK), 0, st,
                                       prev_off, thr_off, (uint32_t)nk, nthr, (const uint2*)nullptr, (const F*)nullptr,
                                       (const F*)nullptr, (const F*)psrc, (F*)pdst, abc.as<F>());
            });
        h->acc_launches = stats.launches;
        h->ms[6] = stats.kernel_ms;
        h->ms[7] = stats.threads;
        h->ms[8] = (double)nterms;
    }
    Ltab.wipe_release();
    ent.release();
    list_off.release();
    cnt.release();
    h->ms[2] = tm.lap();

    // ---- 4. key scalars
    WipeBuf s_vk(std::max<size_t>(lay.n_vk, 1) * 32), s_pk(std::max<size_t>(lay.n_pk, 1) * 32);
    WipeBuf s_ck(std::max<size_t>(n_ck_all, 1) * 32), s_cks(std::max<size_t>(n_ck_all, 1) * 32);
    h->inf_a.alloc(a.nw);
    h->inf_b.alloc(a.nw);
    DevBuf keep_a((a.nw + 1) * 4), keep_b((a.nw + 1) * 4);
    {
        KParams<F> P;
        P.abc = abc.as<F>();
        P.cls = u32(d_cls);
        P.slot = u32(d_slot);
        P.vk_k = s_vk.as<F>();
        P.pk_k = s_pk.as<F>();
        P.ck_k = s_ck.as<F>();
        P.ck_sigma = s_cks.as<F>();
        P.inf_a = h->inf_a.as<uint8_t>();
        P.inf_b = h->inf_b.as<uint8_t>();
        P.keep_a = u32(keep_a);
        P.keep_b = u32(keep_b);
        P.alpha = alpha;
        P.beta = beta;
        P.gamma_inv = gamma_inv;
        P.delta_inv = delta_inv;
        P.sigma = sigma;
        P.nw = (uint32_t)a.nw;
        hipLaunchKernelGGL(k_key_scalars<F>, dim3(grid_for(a.nw + 1, 256)), dim3(256), 0, st, P);
        GG_HIP(hipGetLastError());
    }
    uscan(u32(keep_a), u32(keep_a), a.nw + 1, st, tmp);
    uscan(u32(keep_b), u32(keep_b), a.nw + 1, st, tmp);
    h->nA = rd32(u32(keep_a) + a.nw);
    h->nB = rd32(u32(keep_b) + a.nw);
    WipeBuf s_A(std::max<size_t>(h->nA, 1) * 32), s_B(std::max<size_t>(h->nB, 1) * 32);
    hipLaunchKernelGGL(k_compact<F>, dim3(grid_for(a.nw, 256)), dim3(256), 0, st, (const F*)abc.p,
                       (const uint32_t*)keep_a.p, (uint32_t)a.nw, s_A.as<F>());
    GG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_compact<F>, dim3(grid_for(a.nw, 256)), dim3(256), 0, st, (const F*)abc.p + a.nw,
                       (const uint32_t*)keep_b.p, (uint32_t)a.nw, s_B.as<F>());
    GG_HIP(hipGetLastError());
    WipeBuf s_Z(std::max<size_t>(n - 1, 1) * 32);
    {
        WipeBuf z(n * 32);  // Z_i = (tau^n - 1) delta^-1 tau^i (setup.go:199-210)
        ar.reset();         // the Lagrange phase ended with a stream wait
        hipLaunchKernelGGL(k_fill_geo<F>, dim3(grid_for(n, 256)), dim3(256), 0, st, z.as<F>(), n, zdt, tau);
        GG_HIP(hipGetLastError());
        plk::scan_prod(z.as<F>(), n, st, ar);
        hipLaunchKernelGGL(k_z_brev<F>, dim3(grid_for(n, 256)), dim3(256), 0, st, (const F*)z.p, s_Z.as<F>(),
                           (uint32_t)n, log_n);
        GG_HIP(hipGetLastError());
        GG_WAIT_STREAM(st);
    }
    abc.wipe_release();
    // the single scalars: alpha, beta, delta | beta, delta, gamma, g, -g / sigma
    WipeBuf s_abd(3 * 32), s_g2(5 * 32);
    {
        const F abd[3] = {alpha, beta, delta};
        const F g2s[5] = {beta, delta, gamma, pg, -(pg * inverse(sigma))};
        GG_HIP(hipMemcpyAsync(s_abd.p, abd, sizeof(abd), hipMemcpyHostToDevice, st));
        GG_HIP(hipMemcpyAsync(s_g2.p, g2s, sizeof(g2s), hipMemcpyHostToDevice, st));
        GG_WAIT_STREAM(st);
    }
    h->ms[3] = tm.lap();

    // ---- 5. points
    CombScratch scratch;
    {
        Affine<G1F> g1;
        memcpy(&g1, a.g1, sizeof(g1));
        CombTable<G1F> t1;
        t1.build(g1, st);
        // the scratch at its largest size first: no buffer is replaced between the launches
        const size_t mx1 = std::max({(size_t)3, h->nA, h->nB, h->nZ, lay.n_vk, lay.n_pk, n_ck_all});
        scratch.cur.reserve(mx1 * sizeof(Xyzz<G1F>));
        scratch.prefix.reserve(mx1 * sizeof(G1F));
        auto mul1 = [&](const WipeBuf& s, size_t cnt_, DevBuf& out) {
            out.alloc(std::max<size_t>(cnt_, 1) * sizeof(Affine<G1F>));
            if (cnt_) comb_mul<G1F, FC>(t1, (const F*)s.p, cnt_, out.as<Affine<G1F>>(), scratch, st);
        };
        mul1(s_abd, 3, h->g1_abd);
        mul1(s_A, h->nA, h->g1_A);
        mul1(s_B, h->nB, h->g1_B);
        mul1(s_Z, h->nZ, h->g1_Z);
        mul1(s_vk, lay.n_vk, h->vk_K);
        mul1(s_pk, lay.n_pk, h->g1_K);
        mul1(s_ck, n_ck_all, h->ck);
        mul1(s_cks, n_ck_all, h->ck_sigma);  // basis^sigma = (sigma ckK) G1
        GG_WAIT_STREAM(st);
    }
    h->ms[4] = tm.lap();
    {
        Affine<G2F> g2;
        memcpy(&g2, a.g2, sizeof(g2));
        CombTable<G2F> t2;
        t2.build(g2, st);
        const size_t mx2 = std::max<size_t>(h->nB, 5);
        scratch.cur.reserve(mx2 * sizeof(Xyzz<G2F>));
        scratch.prefix.reserve(mx2 * sizeof(G2F));
        h->g2_B.alloc(std::max<size_t>(h->nB, 1) * sizeof(Affine<G2F>));
        if (h->nB) comb_mul<G2F, FC>(t2, (const F*)s_B.p, h->nB, h->g2_B.as<Affine<G2F>>(), scratch, st);
        h->g2_tail.alloc(5 * sizeof(Affine<G2F>));
        comb_mul<G2F, FC>(t2, (const F*)s_g2.p, 5, h->g2_tail.as<Affine<G2F>>(), scratch, st);
        GG_WAIT_STREAM(st);
    }
    h->ms[5] = tm.lap();
    // the WipeBufs (scalars) and the arena are zeroed as they go out of scope
}

}  // namespace

extern "C" int gg_groth16_setup_layout(size_t n_wires, size_t nb_public, const uint32_t* commitment_wires,
                                       size_t n_commitments, const uint32_t* committed_off,
                                       const uint32_t* committed_wire, uint32_t* wire_class, uint32_t* wire_slot,
                                       size_t* n_vk_k, size_t* n_pk_k, size_t* n_ck) {
    GG_CAPI_BEGIN
    Layout L;
    layout(n_wires, nb_public, commitment_wires, n_commitments, committed_off, committed_wire, L);
    if (wire_class) memcpy(wire_class, L.cls.data(), n_wires * 4);
    if (wire_slot) memcpy(wire_slot, L.slot.data(), n_wires * 4);
    if (n_vk_k) *n_vk_k = L.n_vk;
    if (n_pk_k) *n_pk_k = L.n_pk;
    if (n_ck)
        for (size_t j = 0; j < n_commitments; j++) n_ck[j] = L.n_ck[j];
    GG_CAPI_END
}

extern "C" int gg_groth16_setup(int curve, size_t n_wires, size_t n_constraints, size_t nb_public,
                                const uint32_t* term_off, const uint32_t* term_wire, const uint32_t* term_coeff,
                                const void* coeffs, size_t n_coeffs, const uint32_t* commitment_wires,
                                size_t n_commitments, const uint32_t* committed_off,
                                const uint32_t* committed_wire, const void* tau, const void* alpha,
                                const void* beta, const void* gamma, const void* delta,
                                const void* pedersen_sigma, const void* pedersen_g, const void* omega_mont,
                                const void* g1_gen, const void* g2_gen, gg_g16_setup_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out && term_off && coeffs && tau && alpha && beta && gamma && delta && omega_mont && g1_gen && g2_gen,
             GG_ERR_INVALID_ARG, "null argument");
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG, "unknown curve");
    const SetupArgs a{n_wires,   n_constraints,    nb_public,     n_coeffs,       n_commitments, term_off,
                      term_wire, term_coeff,       commitment_wires, committed_off, committed_wire, coeffs,
                      tau,       alpha,            beta,          gamma,          delta,         pedersen_sigma,
                      pedersen_g, omega_mont,      g1_gen,        g2_gen};
    std::unique_ptr<gg_g16_setup> h(new gg_g16_setup());
    if (curve == GG_CURVE_BN254) run_setup<FrCfg, Fp, Fp2>(a, h.get());
    else run_setup<FrBlsCfg, FpBls, Fp2Bls>(a, h.get());
    *out = h.release();
    GG_CAPI_END
}

extern "C" int gg_groth16_setup_info(gg_g16_setup_t h, int* log_n, size_t* nA, size_t* nB, size_t* nK, size_t* nZ,
                                     size_t* n_vk_k, size_t* n_commitments, size_t* n_ck, size_t n_ck_cap,
                                     size_t* acc_chunk, size_t* acc_launches) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    if (log_n) *log_n = h->log_n;
    if (nA) *nA = h->nA;
    if (nB) *nB = h->nB;
    if (nK) *nK = h->nK;
    if (nZ) *nZ = h->nZ;
    if (n_vk_k) *n_vk_k = h->n_vk;
    if (n_commitments) *n_commitments = h->n_ck.size();
    if (n_ck)
        for (size_t j = 0; j < std::min(n_ck_cap, h->n_ck.size()); j++) n_ck[j] = h->n_ck[j];
    if (acc_chunk) *acc_chunk = h->acc_chunk;
    if (acc_launches) *acc_launches = h->acc_launches;
    GG_CAPI_END
}

extern "C" int gg_groth16_setup_read(gg_g16_setup_t h, int which, void* out_host, size_t bytes) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    const void* src = nullptr;
    size_t want = 0;
    bool host = false;
    const size_t g1 = h->g1b, g2 = h->g2b, ncm = h->n_ck.size();
    auto dev = [&](const DevBuf& b, size_t off, size_t len) {
        src = (const char*)b.p + off;
        want = len;
    };
    if (which >= GG_SETUP_CK_BASIS && which < GG_SETUP_CK_BASIS + 0x100) {
        const size_t j = which - GG_SETUP_CK_BASIS;
        GG_CHECK(j < ncm, GG_ERR_INVALID_ARG, "no such commitment");
        dev(h->ck, h->ck_base[j] * g1, h->n_ck[j] * g1);
    } else if (which >= GG_SETUP_CK_BASIS_SIGMA && which < GG_SETUP_CK_BASIS_SIGMA + 0x100) {
        const size_t j = which - GG_SETUP_CK_BASIS_SIGMA;
        GG_CHECK(j < ncm, GG_ERR_INVALID_ARG, "no such commitment");
        dev(h->ck_sigma, h->ck_base[j] * g1, h->n_ck[j] * g1);
    } else {
        switch (which) {
            case GG_SETUP_G1_A: dev(h->g1_A, 0, h->nA * g1); break;
            case GG_SETUP_G1_B: dev(h->g1_B, 0, h->nB * g1); break;
            case GG_SETUP_G1_K: dev(h->g1_K, 0, h->nK * g1); break;
            case GG_SETUP_G1_Z: dev(h->g1_Z, 0, h->nZ * g1); break;
            case GG_SETUP_G2_B: dev(h->g2_B, 0, h->nB * g2); break;
            case GG_SETUP_ALPHA1: dev(h->g1_abd, 0, g1); break;
            case GG_SETUP_BETA1: dev(h->g1_abd, g1, g1); break;
            case GG_SETUP_DELTA1: dev(h->g1_abd, 2 * g1, g1); break;
            case GG_SETUP_BETA2: dev(h->g2_tail, 0, g2); break;
            case GG_SETUP_DELTA2: dev(h->g2_tail, g2, g2); break;
            case GG_SETUP_GAMMA2: dev(h->g2_tail, 2 * g2, g2); break;
            case GG_SETUP_VK_K: dev(h->vk_K, 0, h->n_vk * g1); break;
            case GG_SETUP_INFINITY_A: dev(h->inf_a, 0, h->nw); break;
            case GG_SETUP_INFINITY_B: dev(h->inf_b, 0, h->nw); break;
            case GG_SETUP_K_WIRE_INDEX:
                src = h->k_wire_index.data();
                want = h->k_wire_index.size() * 4;
                host = true;
                break;
            case GG_SETUP_PEDERSEN_VK:
                GG_CHECK(ncm, GG_ERR_INVALID_ARG, "no Pedersen key: the circuit has no commitments");
                dev(h->g2_tail, 3 * g2, 2 * g2);
                break;
            default: throw Error(GG_ERR_INVALID_ARG, "unknown part " + std::to_string(which));
        }
    }
    GG_CHECK(bytes == want, GG_ERR_INVALID_ARG,
             "part " + std::to_string(which) + " has " + std::to_string(want) + " bytes, caller passed " +
                 std::to_string(bytes));
    if (!want) return GG_OK;
    GG_CHECK(out_host, GG_ERR_INVALID_ARG, "null output");
    if (host) memcpy(out_host, src, want);
    else GG_HIP(hipMemcpy(out_host, src, want, hipMemcpyDeviceToHost));
    GG_CAPI_END
}

extern "C" int gg_groth16_setup_timings(gg_g16_setup_t h, double* ms, int n) {
    GG_CAPI_BEGIN
    GG_CHECK(h && ms, GG_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < std::min(n, GG_SETUP_TIMING_SLOTS); i++) ms[i] = h->ms[i];
    GG_CAPI_END
}

extern "C" int gg_groth16_setup_release(gg_g16_setup_t h) {
    GG_CAPI_BEGIN
    delete h;
    GG_CAPI_END
}

// PlonK Setup on the GPU (backend/plonk/bls12-381/setup.go:108-171 and the same
// file under bn254/): from the sparse R1CS (the arrays of gg_scs_create) and
// the canonical KZG SRS to the trace polynomials, the permutation, the Lagrange
// SRS and -- through the existing key builder -- the proving and verifying key.
// Templated over the scalar field.  No toxic waste here: the SRS is public.
//
//   1. trace (BuildTrace, setup.go:173-225): one thread per row writes Ql, Qr,
//      Qm, Qo, Qk in Lagrange regular form; Qcp_j gets a 1 per committed row.
//   2. permutation (buildPermutation, setup.go:304-358): lro has 3n slots, the
//      unfilled ones hold wire 0.  perm[i] = the greatest j < i with the same
//      wire, or the greatest j overall: a stable radix sort of the slots by wire
//      (rocprim), then every element links to its predecessor in its group and
//      the group's first to its last (found by binary search in the sorted keys).
//   3. S1..S3 (computePermutationPolynomials, setup.go:363-407): a gather from
//      omega^i (running product) times 1, u, u^2.
//   4. canonical forms: inverse NTT (DIF) and bit reversal, as the key does.
//   5. Lagrange SRS: the EC-NTT of ecntt.hip over kzg_g1[:n] unless the caller
//      brought one (setup.go:134).
// Every argument is validated on the host before the first device call.
#include "common.h"
#include "field.cuh"
#include "ecntt.h"
#include "plonk_ops.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gg {
namespace pls {

enum { T_UPLOAD, T_TRACE, T_PERM, T_SGATHER, T_INTT, T_EC_STAGES, T_EC_NORM, T_TOTAL, T_PK_BOUNCE, T_PK_BUILD, T_SLOTS };

// rows i < nb_public: ql = -1; row nb_public + c: the coefficients of constraint
// c (qidx: qL, qR, qO, qM, qC); the padding rows: 0
template <class F>
__global__ void __launch_bounds__(256) k_trace(const uint32_t* qidx, const F* coef, uint32_t n, uint32_t nb_public,
                                               uint32_t ncons, F* ql, F* qr, F* qm, F* qo, F* qk) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F l = F::zero(), r = F::zero(), m = F::zero(), o = F::zero(), k = F::zero();
    if (i < nb_public) {
        l = -F::one();
    } else if (i - nb_public < ncons) {
        const uint32_t* q = qidx + 5 * (size_t)(i - nb_public);
        l = ld_fr(coef + q[0]);
        r = ld_fr(coef + q[1]);
        o = ld_fr(coef + q[2]);
        m = ld_fr(coef + q[3]);
        k = ld_fr(coef + q[4]);
    }
    st_fr(ql + i, l);
    st_fr(qr + i, r);
    st_fr(qm + i, m);
    st_fr(qo + i, o);
    st_fr(qk + i, k);
}
// qcp[nb_public + committed[t]] = 1, t < cnt (committed[t] < ncons checked on the host)
template <class F>
__global__ void __launch_bounds__(256) k_qcp(const uint32_t* committed, uint32_t cnt, uint32_t nb_public, F* qcp) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt) st_fr(qcp + nb_public + committed[t], F::one());
}
// lro (setup.go:316-330) as sort keys, the slot numbers as values
__global__ void __launch_bounds__(256) k_lro(const uint32_t* wires, uint32_t n, uint32_t nb_public, uint32_t ncons,
                                             uint32_t* key, uint32_t* val) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= 3u * n) return;
    const uint32_t col = s / n, i = s - col * n;
    uint32_t w = 0;
    if (i < nb_public) w = col == 0 ? i : 0u;
    else if (i - nb_public < ncons) w = wires[3 * (size_t)(i - nb_public) + col];
    key[s] = w;
    val[s] = s;
}
// sorted (stable) by wire: slot val[p] links to val[p - 1] inside its group, the
// group's first to the group's last (setup.go:334-355)
__global__ void __launch_bounds__(256) k_link(const uint32_t* key, const uint32_t* val, uint32_t m, int64_t* perm) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t k = key[p];
    uint32_t src;
    if (p > 0 && key[p - 1] == k) {
        src = p - 1;
    } else {
        uint32_t lo = p, hi = m;  // key[lo] == k, key[hi] > k (hi == m: past the end)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (key[mid] == k) lo = mid;
            else hi = mid;
        }
        src = lo;
    }
    perm[val[p]] = (int64_t)val[src];
}
template <class F>
__global__ void __launch_bounds__(256) k_fill_geo(F* x, size_t n, F first, F ratio) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_fr(x + i, i ? ratio : first);
}
// S[s] = ID[perm[s]], ID[q] = shift[q div n] * omega^(q mod n); s < 3n
template <class F>
struct Shifts {
    F u[3];
};
template <class F>
__global__ void __launch_bounds__(256) k_sgather(const int64_t* perm, const F* wpow, uint32_t n, uint32_t log_n,
                                                 Shifts<F> sh, F* s1, F* s2, F* s3) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= 3u * n) return;
    const uint32_t q = (uint32_t)perm[s];
    const uint32_t blk = q >> log_n;
    F v = ld_fr(wpow + (q & (n - 1u)));
    if (blk) v = v * sh.u[blk];
    const uint32_t col = s >> log_n, i = s & (n - 1u);
    st_fr((col == 0 ? s1 : col == 1 ? s2 : s3) + i, v);
}

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() {
        auto t1 = std::chrono::steady_clock::now();
        double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};

// initDomains (setup.go:275-290): sizeSystem = n_constraints + nb_public, n its
// next power of two, the big domain 8n for sizeSystem < 6 and 4n otherwise
static void sizes(size_t ncons, size_t nb_public, int* log_n, int* log_big) {
    const size_t size_system = ncons + nb_public;
    GG_CHECK(size_system >= ncons, GG_ERR_INVALID_ARG, "n_constraints + nb_public overflows");
    GG_CHECK(size_system >= 2, GG_ERR_INVALID_ARG,
             "sizeSystem = n_constraints + nb_public = " + std::to_string(size_system) + ": the domain needs n >= 2");
    int lg = 1;
    while (lg < 63 && ((size_t)1 << lg) < size_system) lg++;
    GG_CHECK(lg <= 27, GG_ERR_INVALID_ARG,
             "log_n = " + std::to_string(lg) + " > 27: sizeSystem " + std::to_string(size_system) + " is too large");
    *log_n = lg;
    *log_big = lg + (size_system < 6 ? 3 : 2);
}

struct Args {
    size_t nw, ncons, nb_public, ncoef, n_kzg;
    const uint32_t *wires, *qidx, *coff, *committed;
    const void* coeffs;
    int n_cmt;
    const uint64_t* cmt_idx;
    const void *omega, *u, *kzg, *lag;
};

}  // namespace pls
}  // namespace gg

using namespace gg;
using namespace gg::pls;

struct gg_plonk_setup {
    int curve = 0, log_n = 0, log_big = 0, n_cmt = 0, device = 0, lagrange_computed = 0;
    size_t n = 0, nb_public = 0, pt = 0;
    uint8_t omega[32], u[32];
    std::vector<uint64_t> cmt_idx;
    DevBuf poly[8], qcp[plk::MAX_CMT];  // canonical regular: Ql, Qr, Qm, Qo, Qk, S1, S2, S3
    DevBuf perm, kzg /* n + 3 points */, lag /* n points */;
    double ms[T_SLOTS] = {};
};
using SetupH = struct gg_plonk_setup;  // the tag shares its name with the entry point

namespace {

struct DomainHolder {
    gg_domain_t d = nullptr;
    ~DomainHolder() {
        if (d) (void)gg_domain_release(d);
    }
};
struct PinnedBuf {
    void* p = nullptr;
    explicit PinnedBuf(size_t b) { GG_HIP(hipHostMalloc(&p, std::max<size_t>(b, 16), hipHostMallocDefault)); }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
};

template <class FC>
void run_setup(const Args& a, SetupH* h) {
    using F = Fe<FC>;
    hipStream_t st = hipStreamPerThread;
    Timer tm, total;
    // ---- host checks (before anything touches the device)
    int log_n = 0, log_big = 0;
    sizes(a.ncons, a.nb_public, &log_n, &log_big);
    const size_t n = (size_t)1 << log_n;
    GG_CHECK(a.nw >= 1, GG_ERR_INVALID_ARG, "n_wires is 0");
    GG_CHECK(a.nw < 0xffffffffu, GG_ERR_INVALID_ARG, "n_wires out of range");
    GG_CHECK(a.nb_public <= a.nw, GG_ERR_INVALID_ARG,
             "nb_public " + std::to_string(a.nb_public) + " exceeds n_wires " + std::to_string(a.nw));
    GG_CHECK(a.ncoef >= 1 && a.ncoef < 0xffffffffu, GG_ERR_INVALID_ARG, "empty coefficient table");
    GG_CHECK(a.ncons == 0 || (a.wires && a.qidx), GG_ERR_INVALID_ARG, "null constraint arrays (wires, qidx)");
    for (size_t c = 0; c < a.ncons; c++) {
        for (int k = 0; k < 3; k++)
            if (a.wires[3 * c + k] >= a.nw)
                throw Error(GG_ERR_INVALID_ARG, "constraint " + std::to_string(c) + ": wire id " +
                                                    std::to_string(a.wires[3 * c + k]) + " out of range (n_wires " +
                                                    std::to_string(a.nw) + ")");
        for (int k = 0; k < 5; k++)
            if (a.qidx[5 * c + k] >= a.ncoef)
                throw Error(GG_ERR_INVALID_ARG, "constraint " + std::to_string(c) + ": coefficient id " +
                                                    std::to_string(a.qidx[5 * c + k]) + " out of range (n_coeffs " +
                                                    std::to_string(a.ncoef) + ")");
    }
    if (a.n_cmt) {
        GG_CHECK(a.coff && a.cmt_idx, GG_ERR_INVALID_ARG,
                 "commitments need committed_off and commitment_constraint_indexes");
        GG_CHECK(a.coff[0] == 0, GG_ERR_INVALID_ARG, "committed_off[0] must be 0");
        for (int j = 0; j < a.n_cmt; j++) {
            GG_CHECK(a.coff[j] <= a.coff[j + 1], GG_ERR_INVALID_ARG, "committed_off not monotonic");
            for (uint32_t t = a.coff[j]; t < a.coff[j + 1]; t++) {
                GG_CHECK(a.committed, GG_ERR_INVALID_ARG, "null committed");
                if (a.committed[t] >= a.ncons)
                    throw Error(GG_ERR_INVALID_ARG, "commitment " + std::to_string(j) + ": committed constraint index " +
                                                        std::to_string(a.committed[t]) + " out of range (n_constraints " +
                                                        std::to_string(a.ncons) + ")");
            }
            if (a.nb_public + a.cmt_idx[j] >= n)
                throw Error(GG_ERR_INVALID_ARG, "commitment " + std::to_string(j) + ": nb_public + commitment constraint index " +
                                                    std::to_string(a.cmt_idx[j]) + " is not below n = " + std::to_string(n));
        }
    }
    GG_CHECK(a.n_kzg >= n + 3, GG_ERR_INVALID_ARG,
             "n_kzg = " + std::to_string(a.n_kzg) + " < n + 3 = " + std::to_string(n + 3) + " (setup.go:150)");
    ecntt::check_args(h->curve, log_n, a.omega);
    F omega, u;
    memcpy(&omega, a.omega, 32);
    memcpy(&u, a.u, 32);

    GG_HIP(hipGetDevice(&h->device));
    h->log_n = log_n;
    h->log_big = log_big;
    h->n = n;
    h->n_cmt = a.n_cmt;
    h->nb_public = a.nb_public;
    h->pt = ecntt::point_bytes(h->curve);
    memcpy(h->omega, a.omega, 32);
    memcpy(h->u, a.u, 32);
    h->cmt_idx.assign(a.cmt_idx, a.cmt_idx + a.n_cmt);
    const size_t nb = 32 * n;
    const uint32_t n32 = (uint32_t)n, npub = (uint32_t)a.nb_public, ncons = (uint32_t)a.ncons;

    DevBuf d_wires, d_qidx, d_coef, d_committed;
    upload(d_wires, a.wires, a.ncons * 12, st);
    upload(d_qidx, a.qidx, a.ncons * 20, st);
    upload(d_coef, a.coeffs, a.ncoef * 32, st);
    upload(d_committed, a.committed, a.n_cmt ? (size_t)a.coff[a.n_cmt] * 4 : 0, st);
    upload(h->kzg, a.kzg, (n + 3) * h->pt, st);
    if (a.lag) upload(h->lag, a.lag, n * h->pt, st);
    else h->lag.alloc(n * h->pt);
    GG_WAIT_STREAM(st);
    h->ms[T_UPLOAD] = tm.lap();

    // ---- 1. trace
    for (auto& p : h->poly) p.alloc(nb);
    hipLaunchKernelGGL(k_trace<F>, dim3(grid_for(n, 256)), dim3(256), 0, st, d_qidx.as<uint32_t>(),
                       (const F*)d_coef.p, n32, npub, ncons, h->poly[0].as<F>(), h->poly[1].as<F>(),
                       h->poly[2].as<F>(), h->poly[3].as<F>(), h->poly[4].as<F>());
    GG_HIP(hipGetLastError());
    for (int j = 0; j < a.n_cmt; j++) {
        h->qcp[j].alloc(nb);
        GG_HIP(hipMemsetAsync(h->qcp[j].p, 0, nb, st));
        const uint32_t cnt = a.coff[j + 1] - a.coff[j];
        if (!cnt) continue;
        hipLaunchKernelGGL(k_qcp<F>, dim3(grid_for(cnt, 256)), dim3(256), 0, st,
                           (const uint32_t*)d_committed.p + a.coff[j], cnt, npub, h->qcp[j].as<F>());
        GG_HIP(hipGetLastError());
    }
    GG_WAIT_STREAM(st);
    h->ms[T_TRACE] = tm.lap();

    // ---- 2. permutation
    const uint32_t m = 3u * n32;  // <= 3 * 2^27
    h->perm.alloc((size_t)m * 8);
    {
        DevBuf k0((size_t)m * 4), k1((size_t)m * 4), v0((size_t)m * 4), v1((size_t)m * 4);
        hipLaunchKernelGGL(k_lro, dim3(grid_for(m, 256)), dim3(256), 0, st, (const uint32_t*)d_wires.p, n32, npub,
                           ncons, k0.as<uint32_t>(), v0.as<uint32_t>());
        GG_HIP(hipGetLastError());
        unsigned bits = 1;
        while (bits < 32 && ((size_t)1 << bits) < a.nw) bits++;
        size_t tmp_bytes = 0;
        GG_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k0.as<uint32_t>(), k1.as<uint32_t>(), v0.as<uint32_t>(),
                                         v1.as<uint32_t>(), (size_t)m, 0u, bits, st));
        DevBuf tmp(std::max<size_t>(tmp_bytes, 16));
        GG_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, k0.as<uint32_t>(), k1.as<uint32_t>(), v0.as<uint32_t>(),
                                         v1.as<uint32_t>(), (size_t)m, 0u, bits, st));
        hipLaunchKernelGGL(k_link, dim3(grid_for(m, 256)), dim3(256), 0, st, (const uint32_t*)k1.p,
                           (const uint32_t*)v1.p, m, h->perm.as<int64_t>());
        GG_HIP(hipGetLastError());
        GG_WAIT_STREAM(st);
    }
    h->ms[T_PERM] = tm.lap();

    // ---- 3. S1..S3
    {
        Arena ar;
        ar.reserve(plk::scan_arena_bytes(n) + 4096);
        DevBuf wpow(nb);
        hipLaunchKernelGGL(k_fill_geo<F>, dim3(grid_for(n, 256)), dim3(256), 0, st, wpow.as<F>(), n, F::one(), omega);
        GG_HIP(hipGetLastError());
        plk::scan_prod(wpow.as<F>(), n, st, ar);
        Shifts<F> sh;
        sh.u[0] = F::one();
        sh.u[1] = u;
        sh.u[2] = u * u;
        hipLaunchKernelGGL(k_sgather<F>, dim3(grid_for(m, 256)), dim3(256), 0, st, (const int64_t*)h->perm.p,
                           (const F*)wpow.p, n32, (uint32_t)log_n, sh, h->poly[5].as<F>(), h->poly[6].as<F>(),
                           h->poly[7].as<F>());
        GG_HIP(hipGetLastError());
        GG_WAIT_STREAM(st);
    }
    h->ms[T_SGATHER] = tm.lap();

    // ---- 4. canonical regular forms
    {
        DomainHolder d0;
        int rc = gg_domain_create_ex(h->curve, log_n, a.omega, a.u, &d0.d);
        GG_CHECK(rc == GG_OK, rc, gg_last_error());
        DevBuf t(nb);
        auto canon = [&](DevBuf& b) {
            plk::ntt(d0.d, b.p, 1, 0, 0, st);  // inverse DIF: Lagrange regular -> canonical bit-reversed
            plk::bit_reverse((const F*)b.p, t.as<F>(), n, st);
            GG_HIP(hipMemcpyAsync(b.p, t.p, nb, hipMemcpyDeviceToDevice, st));
        };
        for (auto& p : h->poly) canon(p);
        for (int j = 0; j < a.n_cmt; j++) canon(h->qcp[j]);
        GG_WAIT_STREAM(st);
    }
    h->ms[T_INTT] = tm.lap();

    // ---- 5. Lagrange SRS
    if (!a.lag) {
        double e[2] = {0, 0};
        ecntt::to_lagrange_dev(h->curve, log_n, a.omega, h->kzg.p, h->lag.p, st, e);
        h->ms[T_EC_STAGES] = e[0];
        h->ms[T_EC_NORM] = e[1];
        h->lagrange_computed = 1;
    }
    h->ms[T_TOTAL] = total.lap();
}

}  // namespace

extern "C" int gg_plonk_setup_sizes(size_t n_constraints, size_t nb_public, int* log_n, int* log_big) {
    GG_CAPI_BEGIN
    int a = 0, b = 0;
    sizes(n_constraints, nb_public, &a, &b);
    if (log_n) *log_n = a;
    if (log_big) *log_big = b;
    GG_CAPI_END
}

extern "C" int gg_plonk_setup(int curve, size_t n_wires, size_t n_constraints, size_t nb_public,
                              const uint32_t* wires, const uint32_t* qidx, const void* coeffs, size_t n_coeffs,
                              int n_cmt, const uint32_t* committed_off, const uint32_t* committed,
                              const uint64_t* commitment_constraint_indexes, const void* omega_mont,
                              const void* coset_shift_mont, const void* kzg_g1, size_t n_kzg,
                              const void* kzg_lagrange_g1, gg_plonk_setup_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out && coeffs && omega_mont && coset_shift_mont && kzg_g1, GG_ERR_INVALID_ARG,
             std::string("null argument: ") + (!out ? "out" : !coeffs ? "coeffs" : !omega_mont ? "omega_mont"
                                               : !coset_shift_mont  ? "coset_shift_mont"
                                                                    : "kzg_g1"));
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG,
             "unknown curve " + std::to_string(curve) + " (GG_CURVE_BN254 or GG_CURVE_BLS12_381)");
    GG_CHECK(n_cmt >= 0 && n_cmt <= plk::MAX_CMT, GG_ERR_INVALID_ARG,
             "n_cmt = " + std::to_string(n_cmt) + ": 0 .. 8 BSB22 commitments");
    const Args a{n_wires, n_constraints, nb_public, n_coeffs, n_kzg,  wires,     qidx,           committed_off,
                 committed, coeffs,      n_cmt,     commitment_constraint_indexes, omega_mont, coset_shift_mont,
                 kzg_g1,  kzg_lagrange_g1};
    std::unique_ptr<SetupH> h(new SetupH());
    h->curve = curve;
    if (curve == GG_CURVE_BN254) run_setup<FrCfg>(a, h.get());
    else run_setup<FrBlsCfg>(a, h.get());
    *out = h.release();
    GG_CAPI_END
}

extern "C" int gg_plonk_setup_info(gg_plonk_setup_t h, int* curve, int* log_n, int* log_big, int* n_cmt,
                                   int* lagrange_computed) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    if (curve) *curve = h->curve;
    if (log_n) *log_n = h->log_n;
    if (log_big) *log_big = h->log_big;
    if (n_cmt) *n_cmt = h->n_cmt;
    if (lagrange_computed) *lagrange_computed = h->lagrange_computed;
    GG_CAPI_END
}

extern "C" int gg_plonk_setup_read(gg_plonk_setup_t h, int which, void* out_host, size_t bytes) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    const DevBuf* src = nullptr;
    size_t want = 32 * h->n;
    if (which >= GG_PLONK_SETUP_QL && which <= GG_PLONK_SETUP_S3) {
        src = &h->poly[which - GG_PLONK_SETUP_QL];
    } else if (which >= GG_PLONK_SETUP_QCP && which < GG_PLONK_SETUP_QCP + 0x100) {
        GG_CHECK(which - GG_PLONK_SETUP_QCP < h->n_cmt, GG_ERR_INVALID_ARG, "no such commitment");
        src = &h->qcp[which - GG_PLONK_SETUP_QCP];
    } else if (which == GG_PLONK_SETUP_PERM) {
        src = &h->perm;
        want = 24 * h->n;
    } else if (which == GG_PLONK_SETUP_LAGRANGE) {
        src = &h->lag;
        want = h->pt * h->n;
    } else {
        throw Error(GG_ERR_INVALID_ARG, "unknown part " + std::to_string(which));
    }
    GG_CHECK(bytes == want, GG_ERR_INVALID_ARG,
             "part " + std::to_string(which) + " has " + std::to_string(want) + " bytes, caller passed " +
                 std::to_string(bytes));
    GG_CHECK(out_host, GG_ERR_INVALID_ARG, "null output");
    GG_HIP(hipMemcpy(out_host, src->p, want, hipMemcpyDeviceToHost));
    GG_CAPI_END
}

extern "C" int gg_plonk_setup_timings(gg_plonk_setup_t h, double* ms, int n) {
    GG_CAPI_BEGIN
    GG_CHECK(h && ms, GG_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < std::min(n, (int)T_SLOTS); i++) ms[i] = h->ms[i];
    GG_CAPI_END
}

extern "C" int gg_plonk_setup_pk(gg_plonk_setup_t h, const void* omega_big_mont, int n_devices, const int* devices,
                                 gg_plonk_pk_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(h && omega_big_mont && out, GG_ERR_INVALID_ARG, "null argument");
    GG_CHECK(n_devices <= 1 || devices, GG_ERR_INVALID_ARG, "null devices");
    Timer tm;
    // the key builder takes host buffers: bounce the results through pinned memory
    const size_t n = h->n, nb = 32 * n;
    const int npoly = 8 + h->n_cmt;
    PinnedBuf polys(nb * npoly), perm(24 * n), kzg((n + 3) * h->pt), lag(n * h->pt);
    hipStream_t st = hipStreamPerThread;
    const void* trace[8];
    const void* qcp[plk::MAX_CMT] = {};
    for (int k = 0; k < npoly; k++) {
        void* dst = (char*)polys.p + nb * k;
        const DevBuf& b = k < 8 ? h->poly[k] : h->qcp[k - 8];
        GG_HIP(hipMemcpyAsync(dst, b.p, nb, hipMemcpyDeviceToHost, st));
        if (k < 8) trace[k] = dst;
        else qcp[k - 8] = dst;
    }
    GG_HIP(hipMemcpyAsync(perm.p, h->perm.p, 24 * n, hipMemcpyDeviceToHost, st));
    GG_HIP(hipMemcpyAsync(kzg.p, h->kzg.p, (n + 3) * h->pt, hipMemcpyDeviceToHost, st));
    GG_HIP(hipMemcpyAsync(lag.p, h->lag.p, n * h->pt, hipMemcpyDeviceToHost, st));
    GG_WAIT_STREAM(st);
    h->ms[T_PK_BOUNCE] = tm.lap();
    const uint64_t none = 0;
    int rc = gg_plonk_pk_create_ex(h->curve, h->log_n, h->log_big, h->omega, omega_big_mont, h->u, kzg.p, n + 3, lag.p,
                                   trace, qcp, h->n_cmt, (const int64_t*)perm.p, h->nb_public,
                                   h->n_cmt ? h->cmt_idx.data() : &none, nullptr, n_devices, devices, out);
    h->ms[T_PK_BUILD] = tm.lap();
    if (rc != GG_OK) return rc;  // the message is the key builder's
    GG_CAPI_END
}

extern "C" int gg_plonk_setup_release(gg_plonk_setup_t h) {
    GG_CAPI_BEGIN
    delete h;
    GG_CAPI_END
}

// Sparse-R1CS (PlonK) solver on the GPU: the SCS blueprints' Solve
// (constraint/blueprint_scs.go:53-151, BlueprintGenericSparseR1C and the
// Mul/Add forms it generalises) run level by level as in solver.go:418-533,
// then evaluateLROSmallDomain (constraint/bls12-381/system.go:221-264) builds
// the L, R, O columns the PlonK prover takes (gg_plonk_prove, inputs on
// device).  BLS12-381 fr (PlonK, BASELINE configs[4]) and BN254 fr.  Hint
// calls: gnark's own seven hints run on the GPU too (gg_scs_set_hints,
// hints.cuh); a system with any other hint keeps gnark's host solver.
//
// Constraint c: qL xa + qR xb + qO xc + qM xa xb + qC = 0 with
//   wires[3c + 0..2] = xa, xb, xc and qidx[5c + 0..4] = qL, qR, qO, qM, qC
//   (indices into the coefficient table), flags[c] & 1 = a BSB22 commitment
//   constraint (skipped when solving, blueprint_scs.go:56-60).
// The witness is public then secret at wires 0.. (no ONE_WIRE for SCS,
// solver.go:66-69).  A thread per constraint of a level:
//   xa unsolved: xa = -(qR xb + qO xc + qC) / (qM xb + qL)
//   xb unsolved: xb = -(qL xa + qO xc + qC) / (qM xa + qR)
//   xc unsolved: xc = -(qM xa xb + qL xa + qR xb + qC) / qO
//   all solved:  checkConstraint (blueprint_scs.go:129-151)
// A zero denominator is errDivideByZero.
// This file holds what is the sparse system's own: the constraint arrays, the
// two kernels and the L, R, O columns.  The handle's state, the schedule
// (levels or strands, captured into a HIP graph) and the end of a solve are
// solver_core.h, shared with solver.hip.
#include "solver_core.h"

namespace gg {

template <class C>
struct ScsDev {
    const uint32_t* wires;
    const uint32_t* qidx;
    const uint8_t* flags;
    const Fe<C>* coef;
    const Fe<C>* coef_inv;
    Fe<C>* W;
    uint8_t* solved;
    uint32_t* fail;  // [0] unsatisfied, [1] malformed (two unknowns), [2] division by zero
};

// what scs_step found, for a failure the index of its fail word
enum : int { SCS_OK = -1, SCS_UNSATISFIED = 0, SCS_DIV_ZERO = 2 };

// One constraint with coefficients q[0..4] = qL, qR, qO, qM, qC: pos = 0, 1, 2
// solves for xa, xb, xc (v, from the other two of a, b, o; the unknown's own
// is zero), pos = 3 checks the constraint
template <class C>
__device__ __forceinline__ int scs_step(const ScsDev<C>& d, const uint32_t* q, int pos, const Fe<C>& a,
                                        const Fe<C>& b, const Fe<C>& o, Fe<C>& v) {
    using F = Fe<C>;
    const F qL = ld_fr(d.coef + q[0]), qR = ld_fr(d.coef + q[1]), qM = ld_fr(d.coef + q[3]),
            qC = ld_fr(d.coef + q[4]);
    if (pos <= 1) {
        const F qO = ld_fr(d.coef + q[2]);
        const F den = pos == 0 ? qM * b + qL : qM * a + qR;
        if (den.is_zero()) return SCS_DIV_ZERO;
        const F num = (pos == 0 ? qR * b : qL * a) + qO * o + qC;
        v = -(num * inverse(den));
    } else if (pos == 2) {
        const F qOinv = ld_fr(d.coef_inv + q[2]);
        if (qOinv.is_zero()) return SCS_DIV_ZERO;
        const F t = (qM * a) * b + qL * a + qR * b + qC;
        v = -(t * qOinv);
    } else {
        const F qO = ld_fr(d.coef + q[2]);
        const F t = (qM * a) * b + qL * a + qR * b + qO * o + qC;
        if (!t.is_zero()) return SCS_UNSATISFIED;
    }
    return SCS_OK;
}

template <class C>
__global__ void __launch_bounds__(256) k_scs_level(ScsDev<C> d, const uint32_t* cons, uint32_t count) {
    using F = Fe<C>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = cons[i];
    if (d.flags && (d.flags[c] & 1u)) return;
    const uint32_t xa = d.wires[3 * c], xb = d.wires[3 * c + 1], xc = d.wires[3 * c + 2];
    const bool sa = d.solved[xa], sb = d.solved[xb], sc = d.solved[xc];
    if ((int)!sa + (int)!sb + (int)!sc > 1 || (!sa && xa == xb)) {
        atomicMin(d.fail + 1, c);
        return;
    }
    const int pos = !sa ? 0 : !sb ? 1 : !sc ? 2 : 3;
    const F a = sa ? ld_fr(d.W + xa) : F::zero(), b = sb ? ld_fr(d.W + xb) : F::zero(),
            o = sc ? ld_fr(d.W + xc) : F::zero();
    F v;
    const int bad = scs_step(d, d.qidx + 5 * c, pos, a, b, o, v);
    if (bad != SCS_OK) {
        atomicMin(d.fail + bad, c);
        return;
    }
    if (pos == 3) return;
    const uint32_t w = pos == 0 ? xa : pos == 1 ? xb : xc;
    st_fr(d.W + w, v);
    d.solved[w] = 1;
}

// Strand schedule (strands.h): thread s walks segment s of this launch --
// consecutive constraints of one dependency chain -- in order.  The unknown's
// position is fixed per constraint (unk[c] = 3 c + {0, 1, 2}: xa, xb, xc;
// ~0: none, the constraint is checked), so no solved flags are read; the
// same formulas as k_scs_level.  The chain's last outputs stay in registers.
template <class C>
__global__ void __launch_bounds__(256) k_scs_strands(ScsDev<C> d, const uint32_t* unk, const uint32_t* order,
                                                     const uint32_t* seg_start, uint32_t nseg, uint32_t nin) {
    using F = Fe<C>;
    const uint32_t sg = blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= nseg) return;
    WireCache<F> cache;
    for (uint32_t i = seg_start[sg], e = seg_start[sg + 1]; i < e; i++) {
        const uint32_t c = order[i], u = unk[c];
        const int pos = u == 0xffffffffu ? 3 : (int)(u - 3 * c);
        const uint32_t xa = d.wires[3 * c], xb = d.wires[3 * c + 1], xc = d.wires[3 * c + 2];
        const F a = pos != 0 ? cache.get(xa, d.W, nin) : F::zero(), b = pos != 1 ? cache.get(xb, d.W, nin) : F::zero(),
                o = pos != 2 ? cache.get(xc, d.W, nin) : F::zero();
        F v;
        const int bad = scs_step(d, d.qidx + 5 * c, pos, a, b, o, v);
        if (bad != SCS_OK) {
            atomicMin(d.fail + bad, c);
            if (bad == SCS_DIV_ZERO) return;  // the solve fails: the rest of this strand is never read
            continue;
        }
        if (pos == 3) continue;
        const uint32_t w = pos == 0 ? xa : pos == 1 ? xb : xc;
        st_fr(d.W + w, v);
        d.solved[w] = 1;
        cache.put(w, v);
    }
}

// evaluateLROSmallDomain (system.go:221-264): public placeholder rows, the
// constraints, padding to the power of two -- unused slots carry solution[0]
template <class C>
__global__ void k_scs_lro(const Fe<C>* W, const uint32_t* wires, size_t nb_public, size_t ncons, size_t s,
                          Fe<C>* L, Fe<C>* R, Fe<C>* O) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s) return;
    const Fe<C> s0 = ld_fr(W);
    if (i < nb_public) {
        st_fr(L + i, ld_fr(W + i));
        st_fr(R + i, s0);
        st_fr(O + i, s0);
    } else if (i < nb_public + ncons) {
        const size_t j = i - nb_public;
        st_fr(L + i, ld_fr(W + wires[3 * j]));
        st_fr(R + i, ld_fr(W + wires[3 * j + 1]));
        st_fr(O + i, ld_fr(W + wires[3 * j + 2]));
    } else {
        st_fr(L + i, s0);
        st_fr(R + i, s0);
        st_fr(O + i, s0);
    }
}

}  // namespace gg

using namespace gg;

struct gg_scs : SolverBase {
    size_t nb_public = 0, dom = 0;
    std::vector<uint32_t> h_wires;  // host copies for the strand analysis
    std::vector<uint8_t> h_flags;
    DevBuf wires, qidx, flags, L, R, O;
    bool has_flags = false;
};

namespace {
// the per-level (or per-super-level strand) launches, enqueued on h->st
template <class C>
void enqueue_scs_levels(gg_scs* h) {
    ScsDev<C> d{h->wires.as<uint32_t>(), h->qidx.as<uint32_t>(), h->has_flags ? h->flags.as<uint8_t>() : nullptr,
                h->coef.as<Fe<C>>(), h->coef_inv.as<Fe<C>>(), h->W.as<Fe<C>>(), h->solved.as<uint8_t>(),
                h->fail.as<uint32_t>()};
    enqueue_launches<C>(
        *h,
        [&](const uint32_t* seg_start, uint32_t cnt) {
            hipLaunchKernelGGL(k_scs_strands<C>, dim3(grid_for(cnt, 256)), dim3(256), 0, h->st, d,
                               h->unk.as<uint32_t>(), h->order.as<uint32_t>(), seg_start, cnt,
                               (uint32_t)h->strand_nin);
        },
        [&](const uint32_t* cons, uint32_t cnt) {
            hipLaunchKernelGGL(k_scs_level<C>, dim3(grid_for(cnt, 256)), dim3(256), 0, h->st, d, cons, cnt);
        });
}
}  // namespace

extern "C" int gg_scs_create(int curve, size_t n_wires, size_t n_constraints, size_t nb_public,
                             const uint32_t* wires, const uint32_t* qidx, const uint8_t* flags, const void* coeffs,
                             size_t n_coeffs, const uint32_t* level_off, const uint32_t* level_cons,
                             size_t n_levels, gg_scs_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out && coeffs && level_off, GG_ERR_INVALID_ARG, "null argument");
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG, "unknown curve");
    GG_CHECK(n_wires >= 1 && n_wires < 0xffffffffu && n_constraints < 0xffffffffu && nb_public <= n_wires,
             GG_ERR_INVALID_ARG, "wire / constraint count out of range");
    GG_CHECK(n_coeffs >= 1 && n_coeffs < 0xffffffffu, GG_ERR_INVALID_ARG, "empty coefficient table");
    GG_CHECK(n_constraints == 0 || (wires && qidx && level_cons), GG_ERR_INVALID_ARG, "null constraint arrays");
    for (size_t t = 0; t < 3 * n_constraints; t++)
        GG_CHECK(wires[t] < n_wires, GG_ERR_INVALID_ARG, "wire id out of range");
    for (size_t t = 0; t < 5 * n_constraints; t++)
        GG_CHECK(qidx[t] < n_coeffs, GG_ERR_INVALID_ARG, "coefficient id out of range");
    auto h = std::make_unique<gg_scs>();
    solver_init(*h, curve, 0, n_wires, n_constraints, coeffs, n_coeffs, level_off, level_cons, n_levels);
    h->nb_public = nb_public;
    h->dom = 1;
    while (h->dom < n_constraints + nb_public) h->dom <<= 1;  // ecc.NextPowerOfTwo (system.go:224-225)
    h->h_wires.assign(wires, wires + 3 * n_constraints);
    if (flags) h->h_flags.assign(flags, flags + n_constraints);
    upload(h->wires, wires, 3 * n_constraints * 4);
    upload(h->qidx, qidx, 5 * n_constraints * 4);
    h->has_flags = flags != nullptr;
    if (flags) upload(h->flags, flags, n_constraints);
    h->L.alloc(h->dom * 32);
    h->R.alloc(h->dom * 32);
    h->O.alloc(h->dom * 32);
    *out = h.release();
    GG_CAPI_END
}

extern "C" int gg_scs_release(gg_scs_t h) {
    delete h;
    return GG_OK;
}

extern "C" int gg_scs_info(gg_scs_t h, size_t* n_wires, size_t* n_constraints, size_t* domain) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    if (n_wires) *n_wires = h->nw;
    if (n_constraints) *n_constraints = h->ncons;
    if (domain) *domain = h->dom;
    GG_CAPI_END
}

// newSolver's witness check (constraint/bls12-381/solver.go:71-76) for a
// sparse R1CS: a solve then requires exactly nb_public + nb_secret values
extern "C" int gg_scs_set_inputs(gg_scs_t h, size_t nb_public, size_t nb_secret) {
    GG_CAPI_BEGIN
    GG_CHECK(h && nb_public + nb_secret >= 1 && nb_public + nb_secret <= h->nw, GG_ERR_INVALID_ARG,
             "null handle or input count outside [1, wires]");
    std::lock_guard<std::mutex> lk(h->mu);
    h->expect_inputs = (int64_t)(nb_public + nb_secret);
    GG_CAPI_END
}

extern "C" int gg_scs_solve(gg_scs_t h, const void* witness, size_t n_witness, int witness_on_device, void* w_out,
                            void* l_out, void* r_out, void* o_out, int out_on_device, int64_t* failed) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    GG_CHECK(n_witness >= 1 && n_witness <= h->nw, GG_ERR_INVALID_ARG,
             "witness must hold at least one value (solution[0] pads L, R, O) and fit the wires");
    GG_CHECK(witness, GG_ERR_INVALID_ARG, "null witness");
    if (h->expect_inputs >= 0 && (int64_t)n_witness != h->expect_inputs)
        throw Error(GG_ERR_INVALID_ARG, "invalid witness size, got " + std::to_string(n_witness) + ", expected " +
                                            std::to_string(h->expect_inputs));
    std::lock_guard<std::mutex> lk(h->mu);
    if (failed) *failed = -1;
    // strands (strands.h): commitment rows solve nothing and are left out
    run_schedule(
        *h, witness, n_witness, witness_on_device,
        [&](uint32_t nin) {
            return plan_strands(
                *h, nin,
                [&](uint32_t c, auto&& f) {
                    for (uint32_t k = 0; k < 3; k++) f(3 * c + k, h->h_wires[3 * c + k]);
                },
                [&](uint32_t c) { return h->has_flags && (h->h_flags[c] & 1u); });
        },
        [&] { by_curve(h->curve, [&](auto cfg) { enqueue_scs_levels<decltype(cfg)>(h); }); });
    by_curve(h->curve, [&](auto cfg) {
        using F = Fe<decltype(cfg)>;
        hipLaunchKernelGGL(k_scs_lro<decltype(cfg)>, dim3(grid_for(h->dom, 256)), dim3(256), 0, h->st, h->W.as<F>(),
                           h->wires.as<uint32_t>(), h->nb_public, h->ncons, h->dom, h->L.as<F>(), h->R.as<F>(),
                           h->O.as<F>());
    });
    GG_HIP(hipGetLastError());
    finish_solve(*h, " (the levels do not match the system)", [&](const uint32_t* fail) {
        const uint32_t bad = std::min(fail[0], fail[2]);
        if (bad == 0xffffffffu) return;
        if (failed) *failed = bad;
        throw Error(GG_ERR_UNSATISFIED, "constraint #" + std::to_string(bad) +
                                            (bad == fail[2] ? ": division by zero" : " is not satisfied"));
    });
    const hipMemcpyKind k = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (w_out) GG_HIP(hipMemcpyAsync(w_out, h->W.p, h->nw * 32, k, h->st));
    if (l_out) GG_HIP(hipMemcpyAsync(l_out, h->L.p, h->dom * 32, k, h->st));
    if (r_out) GG_HIP(hipMemcpyAsync(r_out, h->R.p, h->dom * 32, k, h->st));
    if (o_out) GG_HIP(hipMemcpyAsync(o_out, h->O.p, h->dom * 32, k, h->st));
    GG_WAIT_STREAM(h->st);
    GG_CAPI_END
}

extern "C" int gg_scs_solution_dev(gg_scs_t h, void** w, void** l, void** r, void** o) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    if (w) *w = h->W.p;
    if (l) *l = h->L.p;
    if (r) *r = h->R.p;
    if (o) *o = h->O.p;
    GG_CAPI_END
}

extern "C" int gg_scs_schedule(gg_scs_t h, int* strands, size_t* launches, size_t* segments) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    solver_schedule(*h, strands, launches, segments);
    GG_CAPI_END
}

extern "C" int gg_scs_set_hints(gg_scs_t h, size_t n_hints, const uint32_t* hint_id, const uint32_t* in_off,
                                const uint32_t* expr_off, const uint32_t* term_wire, const uint32_t* term_coeff,
                                const uint32_t* out_start, const uint32_t* out_end, const uint32_t* level_off,
                                const uint32_t* level_hints, size_t n_levels) {
    GG_CAPI_BEGIN
    GG_CHECK(h, GG_ERR_INVALID_ARG, "null handle");
    solver_set_hints(*h, n_hints, hint_id, in_off, expr_off, term_wire, term_coeff, out_start, out_end, level_off,
                     level_hints, n_levels);
    GG_CAPI_END
}

// R1CS solver on the GPU: constraint/bn254/solver.go:418-608
// (run + solveR1C), BN254 or BLS12-381 fr (gg_r1cs_create_ex;
// constraint/bls12-381/solver.go is the same code).  Hint calls: gnark's own
// seven hints run on the GPU too (gg_r1cs_set_hints, hints.cuh); a system with
// any other hint keeps gnark's host solver.
//
// The system is handed over once in CSR form -- exactly what gnark's public
// R1CS API yields (r1cs.GetR1Cs() terms, r1cs.Coefficients, r1cs.Levels):
//   term_off[3 c + s] .. term_off[3 c + s + 1]   terms of side s (L, R, O) of c
//   term_wire[t], term_coeff[t]                   wire id and coefficient index
//   coeffs                                        fr table (Montgomery)
//   level_off / level_cons                        r1cs.Levels flattened
// A solve runs one launch per level (constraints of a level are independent,
// solver.go:421-428), a thread per constraint:
//   a, b, c = sum of the solved terms of L, R, O (accumulateInto);
//   at most one unsolved term: its wire gets (c / b - a), (c / a - b) or
//   (a b - c), divided by its coefficient (divByCoeff), and the term joins its
//   side's sum; no unsolved term: a b == c is checked (solver.go:553-571);
//   a zero divisor leaves the wire at 0 after the same check (solver.go:582-601).
// Outputs W (wires) and A, B, C (per-constraint L.w, R.w, O.w: R1CSSolution,
// system.go:269-272) stay in HBM for gg_groth16_prove (inputs_on_device = 1).
// This file holds what is the R1CS's own: the CSR terms, the two kernels and
// A, B, C.  The handle's state, the schedule (levels or strands, captured into
// a HIP graph) and the end of a solve are solver_core.h, shared with
// scs_solver.hip.
#include "solver_core.h"

namespace gg {

template <class FC>
struct R1csDev {
    using Fr = Fe<FC>;
    const uint32_t* off;
    const uint32_t* wire;
    const uint32_t* cidx;
    const Fr* coef;
    const Fr* coef_inv;
    uint32_t ncoef;
    uint32_t one_idx;  // index of the coefficient 1 (CoeffIdOne), ~0 if absent: no product
    uint32_t nin;      // wires < nin are ONE_WIRE + the witness (never written by a solve)
    Fr* W;
    Fr* A;
    Fr* B;
    Fr* C;
    uint8_t* solved;
    uint32_t* fail;  // [0] = first unsatisfied constraint, [1] = first malformed one
};

template <class F>
struct R1csSolved {
    bool ok;
    uint32_t w;  // the unknown's wire
    F val;       // its value as stored
};

// solveR1C's last step for constraint c, whose unknown term ut sits on side
// loc (0, 1, 2: L, R, O) and acc holds the sums of the other terms: the term's
// value joins acc[loc], the wire gets it divided by the term's coefficient
template <class FC>
__device__ __forceinline__ R1csSolved<Fe<FC>> solve_unknown(const R1csDev<FC>& d, uint32_t c, Fe<FC> (&acc)[3],
                                                            int loc, uint32_t ut) {
    using Fr = Fe<FC>;
    bool ok = true;
    Fr v = Fr::zero();
    const Fr a = acc[0], b = acc[1], cc = acc[2];
    if (loc == 0) {
        if (!b.is_zero()) { v = cc * inverse(b) - a; acc[0] = a + v; }
        else ok = a * b == cc;
    } else if (loc == 1) {
        if (!a.is_zero()) { v = cc * inverse(a) - b; acc[1] = b + v; }
        else ok = a * b == cc;
    } else {
        v = a * b - cc;
        acc[2] = cc + v;
    }
    const uint32_t k = d.cidx[ut];
    const Fr kinv = ld_fr(d.coef_inv + k);
    if (kinv.is_zero()) {  // zero coefficient on the unknown: no division possible
        atomicMin(d.fail + 1, c);
        ok = false;
    }
    const uint32_t w = d.wire[ut];
    const Fr val = k == d.one_idx ? v : v * kinv;
    st_fr(d.W + w, val);
    d.solved[w] = 1;
    return {ok, w, val};
}

template <class FC>
__global__ void __launch_bounds__(256) k_solve_level(R1csDev<FC> d, const uint32_t* cons, uint32_t count) {
    using Fr = Fe<FC>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t c = cons[i];
    Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    int loc = -1;
    uint32_t ut = 0;
    bool malformed = false;
    for (int s = 0; s < 3; s++) {
        const uint32_t t0 = d.off[3 * c + s], t1 = d.off[3 * c + s + 1];
        for (uint32_t t = t0; t < t1; t++) {
            const uint32_t w = d.wire[t];
            if (d.solved[w]) {
                const uint32_t k = d.cidx[t];
                acc[s] = acc[s] + (k == d.one_idx ? ld_fr(d.W + w) : ld_fr(d.coef + k) * ld_fr(d.W + w));
                continue;
            }
            if (loc >= 0) malformed = true;  // "found more than one wire to instantiate"
            loc = s;
            ut = t;
        }
    }
    bool ok = true;
    if (malformed) {
        atomicMin(d.fail + 1, c);
        ok = false;
    } else if (loc < 0) {
        ok = acc[0] * acc[1] == acc[2];
    } else {
        ok = solve_unknown(d, c, acc, loc, ut).ok;
    }
    if (!ok) atomicMin(d.fail, c);
    st_fr(d.A + c, acc[0]);
    st_fr(d.B + c, acc[1]);
    st_fr(d.C + c, acc[2]);
}

// Strand schedule (solve_strands): thread s walks segment s of this launch --
// consecutive constraints of one dependency chain -- in order; the unknown
// term of each constraint is known statically (unk[c], ~0 = none), so no
// solved flags are read inside the launch.  Dependencies on other strands were
// solved by earlier launches.
template <class FC>
__global__ void __launch_bounds__(256) k_solve_strands(R1csDev<FC> d, const uint32_t* unk, const uint32_t* order,
                                                       const uint32_t* seg_start, uint32_t nseg) {
    using Fr = Fe<FC>;
    const uint32_t sg = blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= nseg) return;
    WireCache<Fr> cache;
    for (uint32_t i = seg_start[sg], e = seg_start[sg + 1]; i < e; i++) {
        const uint32_t c = order[i], ut = unk[c];
        Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
        int loc = -1;
        for (int s = 0; s < 3; s++) {
            const uint32_t t0 = d.off[3 * c + s], t1 = d.off[3 * c + s + 1];
            for (uint32_t t = t0; t < t1; t++) {
                if (t == ut) {
                    loc = s;
                    continue;
                }
                const uint32_t k = d.cidx[t];
                const Fr x = cache.get(d.wire[t], d.W, d.nin);
                acc[s] = acc[s] + (k == d.one_idx ? x : ld_fr(d.coef + k) * x);
            }
        }
        bool ok = true;
        if (loc < 0) {
            ok = acc[0] * acc[1] == acc[2];
        } else {
            const R1csSolved<Fr> r = solve_unknown(d, c, acc, loc, ut);
            ok = r.ok;
            cache.put(r.w, r.val);
        }
        if (!ok) atomicMin(d.fail, c);
        st_fr(d.A + c, acc[0]);
        st_fr(d.B + c, acc[1]);
        st_fr(d.C + c, acc[2]);
    }
}

}  // namespace gg

using namespace gg;

struct gg_r1cs : SolverBase {
    std::vector<uint32_t> h_off, h_wire;  // host copies for the strand analysis
    DevBuf off, wire, cidx, A, B, C;
};

extern "C" int gg_r1cs_create_ex(int curve, size_t n_wires, size_t n_constraints, const uint32_t* term_off,
                                 const uint32_t* term_wire, const uint32_t* term_coeff, const void* coeffs,
                                 size_t n_coeffs, const uint32_t* level_off, const uint32_t* level_cons,
                                 size_t n_levels, gg_r1cs_t* out) {
    GG_CAPI_BEGIN
    GG_CHECK(out && term_off && coeffs && level_off, GG_ERR_INVALID_ARG, "null argument");
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG, "unknown curve");
    GG_CHECK(n_wires >= 1 && n_wires < 0xffffffffu && n_constraints < 0xffffffffu, GG_ERR_INVALID_ARG,
             "wire / constraint count out of range");
    GG_CHECK(n_coeffs >= 1 && n_coeffs < 0xffffffffu, GG_ERR_INVALID_ARG, "empty coefficient table");
    const size_t nterms = term_off[3 * n_constraints];
    GG_CHECK(term_off[0] == 0, GG_ERR_INVALID_ARG, "term_off[0] must be 0");
    for (size_t i = 0; i < 3 * n_constraints; i++)
        GG_CHECK(term_off[i] <= term_off[i + 1], GG_ERR_INVALID_ARG, "term_off not monotonic");
    GG_CHECK(nterms == 0 || (term_wire && term_coeff), GG_ERR_INVALID_ARG, "null term arrays");
    for (size_t t = 0; t < nterms; t++) {
        GG_CHECK(term_wire[t] < n_wires, GG_ERR_INVALID_ARG, "term wire id out of range");
        GG_CHECK(term_coeff[t] < n_coeffs, GG_ERR_INVALID_ARG, "term coefficient id out of range");
    }
    auto r = std::make_unique<gg_r1cs>();
    solver_init(*r, curve, 1, n_wires, n_constraints, coeffs, n_coeffs, level_off, level_cons, n_levels);
    r->h_off.assign(term_off, term_off + 3 * n_constraints + 1);
    r->h_wire.assign(term_wire, term_wire + nterms);
    upload(r->off, term_off, (3 * n_constraints + 1) * 4);
    upload(r->wire, term_wire, nterms * 4);
    upload(r->cidx, term_coeff, nterms * 4);
    r->A.alloc(std::max<size_t>(n_constraints, 1) * 32);
    r->B.alloc(std::max<size_t>(n_constraints, 1) * 32);
    r->C.alloc(std::max<size_t>(n_constraints, 1) * 32);
    *out = r.release();
    GG_CAPI_END
}

extern "C" int gg_r1cs_create(size_t n_wires, size_t n_constraints, const uint32_t* term_off,
                              const uint32_t* term_wire, const uint32_t* term_coeff, const void* coeffs,
                              size_t n_coeffs, const uint32_t* level_off, const uint32_t* level_cons,
                              size_t n_levels, gg_r1cs_t* out) {
    return gg_r1cs_create_ex(GG_CURVE_BN254, n_wires, n_constraints, term_off, term_wire, term_coeff, coeffs,
                             n_coeffs, level_off, level_cons, n_levels, out);
}

extern "C" int gg_r1cs_release(gg_r1cs_t r) {
    delete r;
    return GG_OK;
}

extern "C" int gg_r1cs_info(gg_r1cs_t r, size_t* n_wires, size_t* n_constraints, size_t* n_levels) {
    GG_CAPI_BEGIN
    GG_CHECK(r, GG_ERR_INVALID_ARG, "null handle");
    if (n_wires) *n_wires = r->nw;
    if (n_constraints) *n_constraints = r->ncons;
    if (n_levels) *n_levels = r->level_off.size() - 1;
    GG_CAPI_END
}

// the per-level (or per-super-level strand) launches, enqueued on r->st
template <class FC>
static void enqueue_levels(gg_r1cs* r) {
    using Fr = Fe<FC>;
    R1csDev<FC> d{r->off.as<uint32_t>(), r->wire.as<uint32_t>(), r->cidx.as<uint32_t>(), r->coef.as<Fr>(),
                  r->coef_inv.as<Fr>(), (uint32_t)r->ncoef, r->one_idx, (uint32_t)r->strand_nin, r->W.as<Fr>(),
                  r->A.as<Fr>(), r->B.as<Fr>(), r->C.as<Fr>(), r->solved.as<uint8_t>(), r->fail.as<uint32_t>()};
    enqueue_launches<FC>(
        *r,
        [&](const uint32_t* seg_start, uint32_t cnt) {
            hipLaunchKernelGGL(k_solve_strands<FC>, dim3(grid_for(cnt, 256)), dim3(256), 0, r->st, d,
                               r->unk.as<uint32_t>(), r->order.as<uint32_t>(), seg_start, cnt);
        },
        [&](const uint32_t* cons, uint32_t cnt) {
            hipLaunchKernelGGL(k_solve_level<FC>, dim3(grid_for(cnt, 256)), dim3(256), 0, r->st, d, cons, cnt);
        });
}

// newSolver's witness check (constraint/bn254/solver.go:71-76): a solve then
// requires exactly nb_public - 1 + nb_secret values (ONE_WIRE is not passed)
extern "C" int gg_r1cs_set_inputs(gg_r1cs_t r, size_t nb_public, size_t nb_secret) {
    GG_CAPI_BEGIN
    GG_CHECK(r && nb_public >= 1, GG_ERR_INVALID_ARG, "null handle or nb_public < 1 (ONE_WIRE)");
    GG_CHECK(nb_public + nb_secret <= r->nw, GG_ERR_INVALID_ARG, "more inputs than wires");
    std::lock_guard<std::mutex> lk(r->mu);
    r->expect_inputs = (int64_t)(nb_public - 1 + nb_secret);
    GG_CAPI_END
}

extern "C" int gg_r1cs_solve(gg_r1cs_t r, const void* witness, size_t n_witness, int witness_on_device,
                             void* w_out, void* a_out, void* b_out, void* c_out, int out_on_device,
                             int64_t* unsatisfied) {
    GG_CAPI_BEGIN
    GG_CHECK(r, GG_ERR_INVALID_ARG, "null handle");
    GG_CHECK(n_witness + 1 <= r->nw, GG_ERR_INVALID_ARG, "witness longer than the wire vector");
    if (r->expect_inputs >= 0 && (int64_t)n_witness != r->expect_inputs)
        throw Error(GG_ERR_INVALID_ARG, "invalid witness size, got " + std::to_string(n_witness) + ", expected " +
                                            std::to_string(r->expect_inputs));
    GG_CHECK(n_witness == 0 || witness, GG_ERR_INVALID_ARG, "null witness");
    std::lock_guard<std::mutex> lk(r->mu);
    if (unsatisfied) *unsatisfied = -1;
    // strands (strands.h): one launch per super-level, a thread per strand
    // segment (the MiMC headline: 65,536 chains, one launch instead of 255)
    run_schedule(
        *r, witness, n_witness, witness_on_device,
        [&](uint32_t nin) {
            return plan_strands(
                *r, nin,
                [&](uint32_t c, auto&& f) {
                    for (uint32_t t = r->h_off[3 * c]; t < r->h_off[3 * c + 3]; t++) f(t, r->h_wire[t]);
                },
                [](uint32_t) { return false; });
        },
        [&] { by_curve(r->curve, [&](auto cfg) { enqueue_levels<decltype(cfg)>(r); }); });
    finish_solve(*r, ", or a zero coefficient on the unknown (the levels do not match the system)",
                 [&](const uint32_t* fail) {
                     if (fail[0] == 0xffffffffu) return;
                     if (unsatisfied) *unsatisfied = fail[0];
                     throw Error(GG_ERR_UNSATISFIED, "constraint #" + std::to_string(fail[0]) + " is not satisfied");
                 });
    const hipMemcpyKind k = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (w_out) GG_HIP(hipMemcpyAsync(w_out, r->W.p, r->nw * 32, k, r->st));
    if (a_out && r->ncons) GG_HIP(hipMemcpyAsync(a_out, r->A.p, r->ncons * 32, k, r->st));
    if (b_out && r->ncons) GG_HIP(hipMemcpyAsync(b_out, r->B.p, r->ncons * 32, k, r->st));
    if (c_out && r->ncons) GG_HIP(hipMemcpyAsync(c_out, r->C.p, r->ncons * 32, k, r->st));
    GG_WAIT_STREAM(r->st);
    GG_CAPI_END
}

// device pointers of the resident solution (valid until the next solve / release)
extern "C" int gg_r1cs_solution_dev(gg_r1cs_t r, void** w, void** a, void** b, void** c) {
    GG_CAPI_BEGIN
    GG_CHECK(r, GG_ERR_INVALID_ARG, "null handle");
    if (w) *w = r->W.p;
    if (a) *a = r->A.p;
    if (b) *b = r->B.p;
    if (c) *c = r->C.p;
    GG_CAPI_END
}

extern "C" int gg_r1cs_schedule(gg_r1cs_t r, int* strands, size_t* launches, size_t* segments) {
    GG_CAPI_BEGIN
    GG_CHECK(r, GG_ERR_INVALID_ARG, "null handle");
    solver_schedule(*r, strands, launches, segments);
    GG_CAPI_END
}

// ---- gnark's built-in hints (hints.cuh) ------------------------------------

extern "C" int gg_hint_supported(uint32_t hint_id, int* supported, const char** go_name) {
    GG_CAPI_BEGIN
    const int k = hint_kind_of(hint_id);
    if (supported) *supported = k >= 0 ? 1 : 0;
    if (go_name) *go_name = k >= 0 ? hint_table()[k].go_name : nullptr;
    GG_CAPI_END
}

extern "C" int gg_hint_eval_host(int curve, uint32_t hint_id, const void* inputs, size_t n_in, void* outputs,
                                 size_t n_out) {
    GG_CAPI_BEGIN
    GG_CHECK(curve == GG_CURVE_BN254 || curve == GG_CURVE_BLS12_381, GG_ERR_INVALID_ARG, "unknown curve");
    const int k = hint_kind_of(hint_id);
    GG_CHECK(k >= 0, GG_ERR_UNSUPPORTED,
             "HintID " + hint_id_hex(hint_id) + " is not one of gnark's built-in hints the GPU solver evaluates");
    const HintInfo& hi = hint_table()[k];
    GG_CHECK((int)n_in == hi.n_in && n_in < 3, GG_ERR_INVALID_ARG,
             std::string(hi.go_name) + " takes " + std::to_string(hi.n_in) + " input(s)");
    GG_CHECK(hi.n_out < 0 || (int)n_out == hi.n_out, GG_ERR_INVALID_ARG,
             std::string(hi.go_name) + " has " + std::to_string(hi.n_out) + " output(s)");
    GG_CHECK(inputs && (outputs || !n_out), GG_ERR_INVALID_ARG, "null argument");
    by_curve(curve, [&](auto cfg) { hint_eval_host<decltype(cfg)>((uint32_t)k, inputs, n_in, outputs, n_out); });
    GG_CAPI_END
}

extern "C" int gg_r1cs_set_hints(gg_r1cs_t r, size_t n_hints, const uint32_t* hint_id, const uint32_t* in_off,
                                 const uint32_t* expr_off, const uint32_t* term_wire, const uint32_t* term_coeff,
                                 const uint32_t* out_start, const uint32_t* out_end, const uint32_t* level_off,
                                 const uint32_t* level_hints, size_t n_levels) {
    GG_CAPI_BEGIN
    GG_CHECK(r, GG_ERR_INVALID_ARG, "null handle");
    solver_set_hints(*r, n_hints, hint_id, in_off, expr_off, term_wire, term_coeff, out_start, out_end, level_off,
                     level_hints, n_levels);
    GG_CAPI_END
}

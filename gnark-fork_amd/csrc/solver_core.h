// What the R1CS solver (solver.hip) and the sparse-R1CS solver
// (scs_solver.hip) share: the handle state, the create-time work, the schedule
// of a solve (witness in, strand plan, the launches captured once into a HIP
// graph per handle -- 256+ tiny launches per solve otherwise) and its tail (the
// unsolved count and the fail words read back).  A solver derives its handle
// from SolverBase and passes what is its own: the strand plan's terms, the
// launches, the text of its errors.
//
// The two systems number their wires differently: an R1CS has ONE_WIRE at wire
// 0 and the witness behind it, a sparse R1CS starts with the witness
// (solver.go:66-69, 103-105).  That is SolverBase::one_wire (1 or 0), and every
// difference that follows from it goes through
//   nin = n_witness + one_wire: the wires solved before the first launch.
#pragma once
#include "common.h"
#include "field.cuh"
#include "hints.cuh"
#include "strands.h"
#include <functional>
#include <mutex>
#include <string>
#include <vector>

namespace gg {

struct SolverBase {
    int device = 0;
    int curve = GG_CURVE_BN254;  // scalar field: BN254 fr or BLS12-381 fr
    int64_t expect_inputs = -1;  // gg_*_set_inputs: required witness length (-1 = not set)
    size_t nw = 0, ncons = 0, ncoef = 0;
    uint32_t one_wire = 0;            // 1: wire 0 is ONE_WIRE (R1CS); 0: the witness starts at wire 0
    uint32_t one_idx = 0xffffffffu;   // index of the coefficient 1 (CoeffIdOne), ~0 if absent
    std::vector<uint32_t> level_off;  // host copy (launch sizes)
    std::vector<uint32_t> h_level_cons;  // host copy for the strand analysis
    // fail: [0] first unsatisfied constraint, [1] first malformed one (or a
    // hint, HINT_FAIL_BIT), [2] first division by zero (SCS); ~0 = none
    DevBuf coef, coef_inv, level_cons, W, solved, fail, inputs, cnt;
    // strand schedule (built at the first solve, per witness length; strands.h)
    long long strand_nin = -1;  // the nin it was built for
    bool strands = false;       // false: the level-by-level launches
    std::vector<uint32_t> sl_seg_off;  // segments of super-level l: [sl_seg_off[l], sl_seg_off[l+1])
    DevBuf unk, order, seg_start;
    size_t n_super = 0, n_seg = 0;
    HintSet hints;  // gg_*_set_hints: a handle with hints runs the level schedule
    bool solved_once = false;
    hipStream_t st = nullptr;
    hipGraphExec_t graph = nullptr;
    std::mutex mu;
    ~SolverBase() {
        if (graph) (void)hipGraphExecDestroy(graph);
        if (st) (void)hipStreamDestroy(st);
    }
};

// f(FrCfg{}) or f(FrBlsCfg{}): the scalar field of a handle's curve
template <class Fn>
void by_curve(int curve, Fn f) {
    if (curve == GG_CURVE_BN254) f(FrCfg{});
    else f(FrBlsCfg{});
}

// Create-time work of a fresh handle: checks that the levels (r1cs.Levels) hold
// every constraint exactly once, inverts the coefficient table on the host
// (divByCoeff: 0 for a zero coefficient) and finds the coefficient 1, uploads
// both and the levels, allocates the solve's buffers and makes the stream.
void solver_init(SolverBase& b, int curve, uint32_t one_wire, size_t n_wires, size_t n_constraints,
                 const void* coeffs, size_t n_coeffs, const uint32_t* level_off, const uint32_t* level_cons,
                 size_t n_levels);

// Uploads a strand plan (strands.h) for nin wires solved up front; terms / skip
// as build_strand_plan takes them.  Returns false (level launches instead) when
// the levels do not match the system; the level kernel then reports it.
template <class Terms, class Skip>
bool plan_strands(SolverBase& b, uint32_t nin, Terms terms, Skip skip) {
    StrandPlan plan;
    if (!build_strand_plan(b.ncons, b.nw, nin, b.level_off, b.h_level_cons, terms, skip, plan))
        return false;
    upload(b.unk, plan.unk.data(), plan.unk.size() * 4);
    upload(b.order, plan.order.data(), plan.order.size() * 4);
    upload(b.seg_start, plan.seg_start.data(), plan.seg_start.size() * 4);
    b.sl_seg_off = std::move(plan.sl_seg_off);
    b.n_seg = plan.seg_start.size() - 1;
    b.n_super = b.sl_seg_off.size() - 1;
    return true;
}

// One solve's launches on b.st, b.mu held: the witness into W (k_solver_init),
// then the schedule -- strands when plan(nin) succeeds (a call of plan_strands;
// GG_SOLVER_LEVELS=1 or hints: the level launches), planned again whenever the
// witness length changes -- whose launches enqueue() issues on b.st: captured
// once into a graph, replayed afterwards.
void run_schedule(SolverBase& b, const void* witness, size_t n_witness, int witness_on_device,
                  const std::function<bool(uint32_t nin)>& plan, const std::function<void()>& enqueue);

// The schedule's launches, for enqueue(): strand(seg_start, count) per
// super-level, or level(cons, count) per level behind the level's hints.
template <class C, class Strand, class Level>
void enqueue_launches(const SolverBase& b, Strand strand, Level level) {
    if (b.strands) {
        for (size_t l = 0; l < b.n_super; l++) {
            const uint32_t a = b.sl_seg_off[l], cnt = b.sl_seg_off[l + 1] - a;
            if (!cnt) continue;
            strand(b.seg_start.as<uint32_t>() + a, cnt);
            GG_HIP(hipGetLastError());
        }
        return;
    }
    for (size_t l = 0; l + 1 < b.level_off.size(); l++) {
        b.hints.enqueue_level<C>(l, b.st, b.coef.as<Fe<C>>(), b.one_idx, b.W.as<Fe<C>>(), b.solved.as<uint8_t>(),
                                 b.fail.as<uint32_t>());
        const uint32_t a = b.level_off[l], cnt = b.level_off[l + 1] - a;
        if (!cnt) continue;
        level(b.level_cons.as<uint32_t>() + a, cnt);
        GG_HIP(hipGetLastError());
    }
}

// The end of a solve: counts the unsolved wires (solver.go:530-532), reads the
// fail words back and raises what they say -- a hint's or a constraint's
// malformed level (fail[1]: "constraint #c: more than one unsolved wire at its
// level" + malformed_suffix), then the solver's own unsatisfied(fail), then
// wires left unsolved.
void finish_solve(SolverBase& b, const std::string& malformed_suffix,
                  const std::function<void(const uint32_t* fail)>& unsatisfied);

// gg_*_schedule and gg_*_set_hints
void solver_schedule(SolverBase& b, int* strands, size_t* launches, size_t* segments);
void solver_set_hints(SolverBase& b, size_t n_hints, const uint32_t* hint_id, const uint32_t* in_off,
                      const uint32_t* expr_off, const uint32_t* term_wire, const uint32_t* term_coeff,
                      const uint32_t* out_start, const uint32_t* out_end, const uint32_t* level_off,
                      const uint32_t* level_hints, size_t n_levels);

// The last RC wires a strand produced, kept in registers: a chain reads its own
// recent outputs (the MiMC rounds: all of them).  Every index below is a
// constant once the loops are unrolled -- get() selects, put() shifts -- which
// keeps cw and cv out of scratch memory (a slot chosen by a counter kept in
// this struct does not: the whole struct then lives in scratch).
template <class F>
struct WireCache {
    static constexpr int RC = 4;
    uint32_t cw[RC] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    F cv[RC];
    // wire w: from the cache, else from W -- wires below nin were written
    // before the launch, any other may be this launch's own store
    __device__ __forceinline__ F get(uint32_t w, const F* W, uint32_t nin) const {
        F x;
        int hit = -1;
#pragma unroll
        for (int q = 0; q < RC; q++)
            if (cw[q] == w) hit = q;
        if (hit >= 0) {
#pragma unroll
            for (int q = 0; q < RC; q++)
                if (q == hit) x = cv[q];
        } else {
            x = w < nin ? ld_fr(W + w) : ld_fr_l2(W + w);
        }
        return x;
    }
    __device__ __forceinline__ void put(uint32_t w, const F& v) {
#pragma unroll
        for (int q = RC - 1; q > 0; q--) {
            cw[q] = cw[q - 1];
            cv[q] = cv[q - 1];
        }
        cw[0] = w;
        cv[0] = v;
    }
};

}  // namespace gg

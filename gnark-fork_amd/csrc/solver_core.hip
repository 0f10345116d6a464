// The host core of the two GPU solvers (solver_core.h): create-time work, the
// schedule of a solve and its tail, and the two kernels that touch only W,
// solved and fail.
#include "solver_core.h"
#include <cstdlib>

namespace gg {

// W <- ONE_WIRE (one_wire = 1: solver.go:103-105), the witness, zeros; wires
// below nin are solved; the fail words are cleared
template <class FC>
__global__ void k_solver_init(Fe<FC>* W, uint8_t* solved, size_t nw, const Fe<FC>* inputs, size_t nin,
                              size_t one_wire, uint32_t* fail) {
    using Fr = Fe<FC>;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) fail[0] = fail[1] = fail[2] = 0xffffffffu;
    if (i >= nw) return;
    if (i < one_wire) st_fr(W + i, Fr::one());
    else if (i < nin) st_fr(W + i, ld_fr(inputs + (i - one_wire)));
    else st_fr(W + i, Fr::zero());
    solved[i] = i < nin ? 1 : 0;
}

// number of unsolved wires (solver.go:530-532)
__global__ void k_count_unsolved(const uint8_t* solved, size_t nw, unsigned long long* cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool u = i < nw && !solved[i];
    const unsigned long long b = __ballot(u);
    if (u && (threadIdx.x & 63) == (uint32_t)(__ffsll(b) - 1)) atomicAdd(cnt, (unsigned long long)__popcll(b));
}

void solver_init(SolverBase& b, int curve, uint32_t one_wire, size_t n_wires, size_t n_constraints,
                 const void* coeffs, size_t n_coeffs, const uint32_t* level_off, const uint32_t* level_cons,
                 size_t n_levels) {
    GG_CHECK(level_off[0] == 0 && level_off[n_levels] == n_constraints, GG_ERR_INVALID_ARG,
             "levels must cover every constraint once");
    GG_CHECK(n_constraints == 0 || level_cons, GG_ERR_INVALID_ARG, "null level_cons");
    std::vector<uint8_t> seen(n_constraints, 0);
    for (size_t l = 0; l < n_levels; l++) {
        GG_CHECK(level_off[l] <= level_off[l + 1], GG_ERR_INVALID_ARG, "level_off not monotonic");
        for (uint32_t i = level_off[l]; i < level_off[l + 1]; i++) {
            const uint32_t c = level_cons[i];
            GG_CHECK(c < n_constraints && !seen[c], GG_ERR_INVALID_ARG, "levels must cover every constraint once");
            seen[c] = 1;
        }
    }
    std::vector<uint8_t> inv(n_coeffs * 32);
    b.one_idx = 0xffffffffu;
    by_curve(curve, [&](auto cfg) {
        using F = Fe<decltype(cfg)>;
        const F* cf = (const F*)coeffs;
        F* out = (F*)inv.data();
        for (size_t i = 0; i < n_coeffs; i++) {
            out[i] = cf[i].is_zero() ? F::zero() : inverse(cf[i]);
            if (b.one_idx == 0xffffffffu && cf[i] == F::one()) b.one_idx = (uint32_t)i;
        }
    });
    GG_HIP(hipGetDevice(&b.device));
    b.curve = curve;
    b.one_wire = one_wire;
    b.nw = n_wires;
    b.ncons = n_constraints;
    b.ncoef = n_coeffs;
    b.level_off.assign(level_off, level_off + n_levels + 1);
    b.h_level_cons.assign(level_cons, level_cons + n_constraints);
    upload(b.coef, coeffs, n_coeffs * 32);
    upload(b.coef_inv, inv.data(), n_coeffs * 32);
    upload(b.level_cons, level_cons, n_constraints * 4);
    b.W.alloc(n_wires * 32);
    b.solved.alloc(n_wires);
    b.fail.alloc(16);
    b.cnt.alloc(16);
    GG_HIP(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
}

void run_schedule(SolverBase& b, const void* witness, size_t n_witness, int witness_on_device,
                  const std::function<bool(uint32_t nin)>& plan, const std::function<void()>& enqueue) {
    const size_t nin = n_witness + b.one_wire;
    GG_CHECK(!b.hints.any() || b.hints.min_out >= nin, GG_ERR_INVALID_ARG,
             "a hint's output range touches a witness wire");
    b.solved_once = true;
    GG_HIP(hipSetDevice(b.device));
    const void* in = witness;
    if (n_witness && !witness_on_device) {
        b.inputs.reserve(n_witness * 32);
        GG_HIP(hipMemcpyAsync(b.inputs.p, witness, n_witness * 32, hipMemcpyHostToDevice, b.st));
        in = b.inputs.p;
    }
    by_curve(b.curve, [&](auto cfg) {
        using F = Fe<decltype(cfg)>;
        hipLaunchKernelGGL(k_solver_init<decltype(cfg)>, dim3(grid_for(b.nw, 256)), dim3(256), 0, b.st, b.W.as<F>(),
                           b.solved.as<uint8_t>(), b.nw, (const F*)in, nin, (size_t)b.one_wire,
                           b.fail.as<uint32_t>());
    });
    GG_HIP(hipGetLastError());
    // schedule: strands when the levels allow it (GG_SOLVER_LEVELS=1: level launches)
    if (b.strand_nin != (long long)nin) {
        const bool levels_only = getenv("GG_SOLVER_LEVELS") && atoi(getenv("GG_SOLVER_LEVELS"));
        b.strands = !levels_only && !b.hints.any() && plan((uint32_t)nin);
        b.strand_nin = (long long)nin;
        if (b.graph) {
            (void)hipGraphExecDestroy(b.graph);
            b.graph = nullptr;
        }
    }
    // the launches: captured once into a graph, replayed afterwards
    if (!b.graph) {
        hipGraph_t g;
        GG_HIP(hipStreamBeginCapture(b.st, hipStreamCaptureModeThreadLocal));
        try {
            enqueue();
        } catch (...) {
            (void)hipStreamEndCapture(b.st, &g);
            throw;
        }
        GG_HIP(hipStreamEndCapture(b.st, &g));
        hipError_t e = hipGraphInstantiate(&b.graph, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        GG_HIP(e);
    }
    GG_HIP(hipGraphLaunch(b.graph, b.st));
}

void finish_solve(SolverBase& b, const std::string& malformed_suffix,
                  const std::function<void(const uint32_t* fail)>& unsatisfied) {
    GG_HIP(hipMemsetAsync(b.cnt.p, 0, 8, b.st));
    hipLaunchKernelGGL(k_count_unsolved, dim3(grid_for(b.nw, 256)), dim3(256), 0, b.st, b.solved.as<uint8_t>(),
                       b.nw, b.cnt.as<unsigned long long>());
    GG_HIP(hipGetLastError());
    uint32_t fail[3];
    unsigned long long unsolved = 0;
    GG_HIP(hipMemcpyAsync(fail, b.fail.p, 12, hipMemcpyDeviceToHost, b.st));
    GG_HIP(hipMemcpyAsync(&unsolved, b.cnt.p, 8, hipMemcpyDeviceToHost, b.st));
    GG_WAIT_STREAM(b.st);
    GG_CHECK(fail[1] == 0xffffffffu || !(fail[1] & HINT_FAIL_BIT) || !b.hints.any(), GG_ERR_INVALID_ARG,
             hint_unsolved_message(fail[1]));
    GG_CHECK(fail[1] == 0xffffffffu, GG_ERR_INVALID_ARG,
             "constraint #" + std::to_string(fail[1]) + ": more than one unsolved wire at its level" +
                 malformed_suffix);
    unsatisfied(fail);
    GG_CHECK(unsolved == 0, GG_ERR_UNSATISFIED,
             "solver didn't assign a value to all wires (" + std::to_string(unsolved) + " left)");
}

void solver_schedule(SolverBase& b, int* strands, size_t* launches, size_t* segments) {
    std::lock_guard<std::mutex> lk(b.mu);
    size_t nl = 0;
    if (b.strands) {
        for (size_t l = 0; l < b.n_super; l++) nl += b.sl_seg_off[l + 1] > b.sl_seg_off[l];
    } else {
        for (size_t l = 0; l + 1 < b.level_off.size(); l++) nl += b.level_off[l + 1] > b.level_off[l];
        nl += b.hints.launches();
    }
    if (strands) *strands = b.strands ? 1 : 0;
    if (launches) *launches = nl;
    if (segments) *segments = b.strands ? b.n_seg : 0;
}

void solver_set_hints(SolverBase& b, size_t n_hints, const uint32_t* hint_id, const uint32_t* in_off,
                      const uint32_t* expr_off, const uint32_t* term_wire, const uint32_t* term_coeff,
                      const uint32_t* out_start, const uint32_t* out_end, const uint32_t* level_off,
                      const uint32_t* level_hints, size_t n_levels) {
    std::lock_guard<std::mutex> lk(b.mu);
    GG_CHECK(!b.solved_once, GG_ERR_INVALID_ARG, "set_hints: the handle has already solved");
    GG_HIP(hipSetDevice(b.device));
    // wires below nin are ONE_WIRE / the witness (gg_*_set_inputs, when called)
    const size_t first_internal = (b.expect_inputs >= 0 ? (size_t)b.expect_inputs : 0) + b.one_wire;
    b.hints.init(b.nw, b.ncoef, b.ncons, first_internal, b.level_off.size() - 1, n_hints, hint_id, in_off, expr_off,
                 term_wire, term_coeff, out_start, out_end, level_off, level_hints, n_levels);
}

}  // namespace gg

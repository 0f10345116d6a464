// gnark's built-in hints for the GPU solvers (solver.hip, scs_solver.hip):
// the seven hint functions gnark itself registers, recognised by their HintID
// (FNV-1a-32 of the Go function name, constraint/solver/hint.go:87-96) and
// evaluated inside the level loop as solveWithHint does
// (constraint/bn254/solver.go:197-246): every input is a linear expression
// over solved wires, taken out of Montgomery form to the integer in [0, r);
// every output goes back into Montgomery form and its wire is marked solved.
//
//   InvZeroHint       1 / 1    1/a mod r, 0 for a = 0   (solver/hint_registry.go:77-90)
//   ithBit            2 / 1    bit inputs[1] of inputs[0] (std/math/bits/hints.go:26-35)
//   nBits             1 / any  out[i] = bit i             (hints.go:39-45)
//   nTrits            1 / any  out[i] = base-3 digit i    (hints.go:49-63)
//   nNaf              1 / any  NAF digits 0, 1, -1        (hints.go:67-114)
//   minOutputHint     2 / 1    a if cmpInField(a, b) == -1 else b (std/math/cmp/bounded.go:192-214)
//   isLessOutputHint  2 / 1    1 if cmpInField(a, b) == -1 else 0 (bounded.go:217-229)
//
// The arithmetic is written once as GG_HD functions (the host entry point
// gg_hint_eval_host and the kernels run the same code).  Two kernels per level
// that holds hints:
//   k_hint_eval     a thread per hint: the inputs, then a 64-byte packed result
//                   (the field element; the canonical value for nBits; 2-bit
//                   digits for nTrits / nNaf, which are sequential by nature);
//   k_hint_scatter  a thread per output wire of the level: the hint through a
//                   binary search in the level's prefix of output counts, the
//                   digit decoded, the Montgomery constant stored -- lanes of a
//                   wave write consecutive 32-byte wires.
// Both touch only W, solved and fail, so one implementation serves both solvers.
#pragma once
#include "common.h"
#include "field.cuh"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace gg {

enum : uint32_t {
    HINT_INV_ZERO = 0,
    HINT_ITH_BIT = 1,
    HINT_NBITS = 2,
    HINT_NTRITS = 3,
    HINT_NNAF = 4,
    HINT_MIN = 5,
    HINT_IS_LESS = 6,
    HINT_KINDS = 7
};
// a term of a hint input with this wire id is a constant: the coefficient alone
// (Term.IsConstant; an R1CS caller may equally pass coefficient x wire 0)
constexpr uint32_t HINT_CONST_WIRE = 0xffffffffu;
// fail[1] of a solve: the hint's index with this bit set (a constraint id otherwise)
constexpr uint32_t HINT_FAIL_BIT = 0x80000000u;

struct HintInfo {
    uint32_t id;
    const char* go_name;
    int n_in;
    int n_out;  // -1: any
};
inline const HintInfo* hint_table() {
    static const HintInfo t[HINT_KINDS] = {
        {0x970c3c2fu, "github.com/consensys/gnark/constraint/solver.InvZeroHint", 1, 1},
        {0xcc606925u, "github.com/consensys/gnark/std/math/bits.ithBit", 2, 1},
        {0xf54cdbebu, "github.com/consensys/gnark/std/math/bits.nBits", 1, -1},
        {0x7f90a7adu, "github.com/consensys/gnark/std/math/bits.nTrits", 1, -1},
        {0x5ca55ec0u, "github.com/consensys/gnark/std/math/bits.nNaf", 1, -1},
        {0x7970dda3u, "github.com/consensys/gnark/std/math/cmp.minOutputHint", 2, 1},
        {0x73e09b3cu, "github.com/consensys/gnark/std/math/cmp.isLessOutputHint", 2, 1},
    };
    return t;
}
inline int hint_kind_of(uint32_t id) {
    for (int k = 0; k < (int)HINT_KINDS; k++)
        if (hint_table()[k].id == id) return k;
    return -1;
}
inline std::string hint_id_hex(uint32_t id) {
    char buf[16];
    snprintf(buf, sizeof buf, "0x%08x", id);
    return buf;
}

// ---- the arithmetic (host and device) -------------------------------------

// -1, 0, 1: big.Int.Cmp of two 256-bit integers (8 x u32, little endian)
GG_HD int hint_cmp256(const uint32_t* a, const uint32_t* b) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (a[i] != b[i]) r = a[i] < b[i] ? -1 : 1;
    return r;
}

// cmpInField (bounded.go:193-199) on canonical values: the order flips when
// the two sit strictly on opposite sides of r >> 1
template <class C>
GG_HD int hint_cmp_in_field(const uint32_t* a, const uint32_t* b) {
    uint32_t half[8];
#pragma unroll
    for (int i = 0; i < 8; i++) half[i] = (C::P[i] >> 1) | (i < 7 ? C::P[i < 7 ? i + 1 : 7] << 31 : 0u);
    const int c = hint_cmp256(a, b);
    return hint_cmp256(a, half) * hint_cmp256(b, half) == -1 ? -c : c;
}

// base-3 digits of a 256-bit integer, 2 bits each, digit i at bit 2 i of the
// 512-bit result: 3^16 splits off sixteen digits (one word) per long division;
// 2^256 < 3^162, so eleven words hold every digit
GG_HD void hint_trits(const uint32_t* canon, uint32_t* packed) {
    constexpr uint32_t D = 43046721u;  // 3^16
    uint32_t n[8];
#pragma unroll
    for (int i = 0; i < 8; i++) n[i] = canon[i];
#pragma unroll 1
    for (int w = 0; w < 16; w++) {
        uint32_t word = 0;
        if (w < 11) {
            uint64_t rem = 0;
#pragma unroll
            for (int i = 7; i >= 0; i--) {
                const uint64_t cur = (rem << 32) | n[i];
                n[i] = (uint32_t)(cur / D);
                rem = cur % D;
            }
            uint32_t r = (uint32_t)rem;
            for (int k = 0; k < 16; k++) {
                word |= (r % 3u) << (2 * k);
                r /= 3u;
            }
        }
        packed[w] = word;
    }
}

// nafDecomposition (hints.go:73-114), 2 bits per digit (0, 1, 2 = -1): an odd
// value ending in binary 11 gives -1 and is rounded up before the shift.  A
// value below 2^255 has at most 256 digits, and the rounding never leaves 256 bits.
GG_HD void hint_naf(const uint32_t* canon, uint32_t* packed) {
    uint32_t a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = canon[i];
#pragma unroll 1
    for (int w = 0; w < 16; w++) {
        uint32_t word = 0;
        for (int k = 0; k < 16; k++) {
            uint32_t d = 0;
            if (a[0] & 1u) {
                d = 1;
                if ((a[0] & 3u) == 3u) {
                    d = 2;
                    uint32_t c = 1;
#pragma unroll
                    for (int i = 0; i < 8; i++) a[i] = __builtin_addc(a[i], 0u, c, &c);
                }
            }
            word |= d << (2 * k);
#pragma unroll
            for (int i = 0; i < 8; i++) a[i] = (a[i] >> 1) | (i < 7 ? a[i < 7 ? i + 1 : 7] << 31 : 0u);
        }
        packed[w] = word;
    }
}

// a hint's packed result (16 words, written word by word: the kernel passes
// its slot in global memory) from its inputs x0, x1 (Montgomery; x1 unused by
// the one-input hints)
template <class C>
GG_HD void hint_eval(uint32_t kind, const Fe<C>& x0, const Fe<C>& x1, uint32_t* out) {
    static_assert(C::N == 8, "scalar fields of 8 limbs");
    Fe<C> res = Fe<C>::zero();
    const Fe<C> c0 = from_mont(x0);
    if (kind == HINT_NBITS) {
        res = c0;  // the canonical value: the scatter picks its bits
    } else if (kind == HINT_NTRITS) {
        hint_trits(c0.v, out);
        return;
    } else if (kind == HINT_NNAF) {
        hint_naf(c0.v, out);
        return;
    } else if (kind == HINT_INV_ZERO) {
        res = inverse(x0);  // 0 for 0
    } else if (kind == HINT_ITH_BIT) {
        // inputs[0].Bit(inputs[1]); 0 when the index is no uint64.  An index in
        // [2^63, 2^64) is 0 here as well (the reference's int() goes negative
        // there and big.Int.Bit panics)
        const Fe<C> c1 = from_mont(x1);
        uint32_t hi = 0;
#pragma unroll
        for (int i = 1; i < 8; i++) hi |= c1.v[i];
        uint32_t bit = 0;
        if (hi == 0 && c1.v[0] < 256u) {
            const uint32_t i = c1.v[0];
#pragma unroll
            for (int k = 0; k < 8; k++)
                if ((i >> 5) == (uint32_t)k) bit = (c0.v[k] >> (i & 31u)) & 1u;
        }
        if (bit) res = Fe<C>::one();
    } else {  // HINT_MIN, HINT_IS_LESS
        const Fe<C> c1 = from_mont(x1);
        const bool less = hint_cmp_in_field<C>(c0.v, c1.v) == -1;
        if (kind == HINT_MIN) res = less ? x0 : x1;
        else if (less) res = Fe<C>::one();
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        out[i] = res.v[i];
        out[8 + i] = 0;
    }
}

// true: the packed result is the (single) output itself
GG_HD bool hint_is_field(uint32_t kind) { return kind != HINT_NBITS && kind != HINT_NTRITS && kind != HINT_NNAF; }

// output j of a digit hint as a code: 0, 1, 2 or 3 (= -1)
GG_HD uint32_t hint_digit(uint32_t kind, const uint32_t* packed, uint32_t j) {
    if (j >= 256u) return 0;  // past every digit of a value below 2^256
    if (kind == HINT_NBITS) return (packed[j >> 5] >> (j & 31u)) & 1u;
    const uint32_t d = (packed[j >> 4] >> (2u * (j & 15u))) & 3u;
    return kind == HINT_NNAF && d == 2u ? 3u : d;
}
template <class C>
GG_HD Fe<C> hint_const(uint32_t code) {
    const Fe<C> one = Fe<C>::one();
    if (code == 0) return Fe<C>::zero();
    if (code == 1) return one;
    return code == 2 ? one + one : -one;
}

// ---- the kernels ----------------------------------------------------------

template <class C>
struct HintDev {
    const uint32_t* kind;        // per hint
    const uint32_t* in_off;      // inputs of hint h: [in_off[h], in_off[h + 1])
    const uint32_t* expr_off;    // terms of input e: [expr_off[e], expr_off[e + 1])
    const uint32_t* term_wire;
    const uint32_t* term_coeff;  // into coef
    const uint32_t* out_start;   // per hint
    const uint32_t* lvl_hints;   // the hints in level order
    const uint32_t* lvl_pref;    // outputs before position p of lvl_hints (n_hints + 1)
    uint32_t* packed;            // 16 words per position of lvl_hints
    const Fe<C>* coef;
    uint32_t one_idx;            // index of the coefficient 1, ~0 if absent: no product
    Fe<C>* W;
    uint8_t* solved;
    uint32_t* fail;
};

// positions [first, first + count) of lvl_hints: one level's hints
template <class C>
__global__ void __launch_bounds__(256) k_hint_eval(HintDev<C> d, uint32_t first, uint32_t count) {
    using F = Fe<C>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t pos = first + i, h = d.lvl_hints[pos];
    F x0 = F::zero(), x1 = F::zero();
    bool unsolved = false;
    const uint32_t e0 = d.in_off[h], e1 = d.in_off[h + 1];
    for (uint32_t e = e0; e < e1; e++) {
        F acc = F::zero();
        for (uint32_t t = d.expr_off[e], te = d.expr_off[e + 1]; t < te; t++) {
            const uint32_t w = d.term_wire[t], k = d.term_coeff[t];
            if (w == HINT_CONST_WIRE) {
                acc = acc + ld_fr(d.coef + k);
                continue;
            }
            if (!d.solved[w]) {
                unsolved = true;
                continue;
            }
            acc = acc + (k == d.one_idx ? ld_fr(d.W + w) : ld_fr(d.coef + k) * ld_fr(d.W + w));
        }
        if (e == e0) x0 = acc;
        else x1 = acc;
    }
    uint32_t* out = d.packed + 16 * (size_t)pos;
    if (unsolved) {  // the levels do not match the system
        atomicMin(d.fail + 1, HINT_FAIL_BIT | h);
        st_fr(reinterpret_cast<F*>(out), F::zero());
        st_fr(reinterpret_cast<F*>(out) + 1, F::zero());
    } else {
        hint_eval<C>(d.kind[h], x0, x1, out);
    }
}

// a thread per output wire of the level: n_out = lvl_pref[first + count] - lvl_pref[first]
template <class C>
__global__ void __launch_bounds__(256) k_hint_scatter(HintDev<C> d, uint32_t first, uint32_t count, uint32_t n_out) {
    using F = Fe<C>;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_out) return;
    const uint32_t* pref = d.lvl_pref + first;
    const uint32_t target = pref[0] + t;
    // the last position whose prefix is <= target (pref[count] > target): a
    // hint without outputs shares its prefix with the next one and is passed over
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pref[mid] <= target) lo = mid;
        else hi = mid;
    }
    const uint32_t pos = first + lo, h = d.lvl_hints[pos], j = target - pref[lo], kind = d.kind[h];
    const uint32_t* pk = d.packed + 16 * (size_t)pos;
    const F v = hint_is_field(kind) ? ld_fr(reinterpret_cast<const F*>(pk)) : hint_const<C>(hint_digit(kind, pk, j));
    const uint32_t w = d.out_start[h] + j;
    st_fr(d.W + w, v);
    d.solved[w] = 1;
}

// ---- host side: a handle's hints (gg_r1cs_set_hints / gg_scs_set_hints) ----

struct HintSet {
    bool set = false;  // set_hints was called (at most once)
    size_t n = 0;
    uint32_t min_out = 0xffffffffu;   // the lowest output wire
    std::vector<uint32_t> level_off;  // positions of level l: [level_off[l], level_off[l + 1])
    std::vector<uint32_t> pref;       // host copy of lvl_pref
    DevBuf kind, in_off, expr_off, term_wire, term_coeff, out_start, lvl_hints, lvl_pref, packed;

    bool any() const { return n > 0; }

    // Validates and uploads.  first_internal: wires below it are inputs (never
    // an output); handle_levels: the handle's level count.
    void init(size_t n_wires, size_t n_coeffs, size_t n_constraints, size_t first_internal, size_t handle_levels,
              size_t n_hints, const uint32_t* hint_id, const uint32_t* h_in_off, const uint32_t* h_expr_off,
              const uint32_t* h_term_wire, const uint32_t* h_term_coeff, const uint32_t* h_out_start,
              const uint32_t* h_out_end, const uint32_t* h_level_off, const uint32_t* h_level_hints,
              size_t n_levels) {
        GG_CHECK(!set, GG_ERR_INVALID_ARG, "set_hints: the handle's hints are already set");
        GG_CHECK(n_levels == handle_levels, GG_ERR_INVALID_ARG,
                 "set_hints: " + std::to_string(n_levels) + " levels, the handle has " +
                     std::to_string(handle_levels));
        GG_CHECK(n_hints < HINT_FAIL_BIT && n_constraints < HINT_FAIL_BIT, GG_ERR_INVALID_ARG,
                 "set_hints: hint / constraint count out of range");
        GG_CHECK(h_level_off, GG_ERR_INVALID_ARG, "set_hints: null level_off");
        if (n_hints)
            GG_CHECK(hint_id && h_in_off && h_expr_off && h_out_start && h_out_end && h_level_hints,
                     GG_ERR_INVALID_ARG, "set_hints: null argument");
        std::vector<uint32_t> kinds(n_hints);
        for (size_t h = 0; h < n_hints; h++) {
            const int k = hint_kind_of(hint_id[h]);
            GG_CHECK(k >= 0, GG_ERR_UNSUPPORTED,
                     "hint #" + std::to_string(h) + ": HintID " + hint_id_hex(hint_id[h]) +
                         " is not one of gnark's built-in hints the GPU solver evaluates");
            kinds[h] = (uint32_t)k;
        }
        // arities (the Go functions would index out of range) and term indices
        size_t n_expr = 0, n_terms = 0;
        if (n_hints) {
            GG_CHECK(h_in_off[0] == 0, GG_ERR_INVALID_ARG, "set_hints: in_off[0] must be 0");
            for (size_t h = 0; h < n_hints; h++) {
                GG_CHECK(h_in_off[h] <= h_in_off[h + 1], GG_ERR_INVALID_ARG, "set_hints: in_off not monotonic");
                const HintInfo& hi = hint_table()[kinds[h]];
                GG_CHECK((int)(h_in_off[h + 1] - h_in_off[h]) == hi.n_in, GG_ERR_INVALID_ARG,
                         "hint #" + std::to_string(h) + " (" + hi.go_name + "): takes " + std::to_string(hi.n_in) +
                             " input(s)");
                GG_CHECK(h_out_start[h] <= h_out_end[h], GG_ERR_INVALID_ARG,
                         "hint #" + std::to_string(h) + ": out_start > out_end");
                GG_CHECK(hi.n_out < 0 || (int)(h_out_end[h] - h_out_start[h]) == hi.n_out, GG_ERR_INVALID_ARG,
                         "hint #" + std::to_string(h) + " (" + hi.go_name + "): has " + std::to_string(hi.n_out) +
                             " output(s)");
            }
            n_expr = h_in_off[n_hints];
            GG_CHECK(h_expr_off[0] == 0, GG_ERR_INVALID_ARG, "set_hints: expr_off[0] must be 0");
            for (size_t e = 0; e < n_expr; e++)
                GG_CHECK(h_expr_off[e] <= h_expr_off[e + 1], GG_ERR_INVALID_ARG, "set_hints: expr_off not monotonic");
            n_terms = h_expr_off[n_expr];
            GG_CHECK(n_terms == 0 || (h_term_wire && h_term_coeff), GG_ERR_INVALID_ARG, "set_hints: null term arrays");
            for (size_t t = 0; t < n_terms; t++) {
                GG_CHECK(h_term_wire[t] < n_wires || h_term_wire[t] == HINT_CONST_WIRE, GG_ERR_INVALID_ARG,
                         "set_hints: term wire id out of range");
                GG_CHECK(h_term_coeff[t] < n_coeffs, GG_ERR_INVALID_ARG, "set_hints: term coefficient id out of range");
            }
        }
        // output ranges: above the inputs, inside the wires, disjoint
        std::vector<std::pair<uint32_t, uint32_t>> ranges;
        uint32_t lowest = 0xffffffffu;
        for (size_t h = 0; h < n_hints; h++) {
            if (h_out_start[h] == h_out_end[h]) continue;
            GG_CHECK(h_out_start[h] >= first_internal, GG_ERR_INVALID_ARG,
                     "hint #" + std::to_string(h) + ": output range touches an input wire");
            GG_CHECK(h_out_end[h] <= n_wires, GG_ERR_INVALID_ARG,
                     "hint #" + std::to_string(h) + ": output range passes the wires");
            ranges.emplace_back(h_out_start[h], h_out_end[h]);
            lowest = std::min(lowest, h_out_start[h]);
        }
        std::sort(ranges.begin(), ranges.end());
        for (size_t i = 1; i < ranges.size(); i++)
            GG_CHECK(ranges[i - 1].second <= ranges[i].first, GG_ERR_INVALID_ARG,
                     "set_hints: output ranges overlap at wire " + std::to_string(ranges[i].first));
        // every hint in exactly one level
        GG_CHECK(h_level_off[0] == 0 && h_level_off[n_levels] == n_hints, GG_ERR_INVALID_ARG,
                 "set_hints: levels must hold every hint once");
        std::vector<uint8_t> seen(n_hints, 0);
        std::vector<uint32_t> pf(n_hints + 1, 0);
        for (size_t l = 0; l < n_levels; l++) {
            GG_CHECK(h_level_off[l] <= h_level_off[l + 1] && h_level_off[l + 1] <= n_hints, GG_ERR_INVALID_ARG,
                     "set_hints: level_off not monotonic");
            for (uint32_t i = h_level_off[l]; i < h_level_off[l + 1]; i++) {
                const uint32_t h = h_level_hints[i];
                GG_CHECK(h < n_hints && !seen[h], GG_ERR_INVALID_ARG, "set_hints: levels must hold every hint once");
                seen[h] = 1;
                pf[i + 1] = pf[i] + (h_out_end[h] - h_out_start[h]);
            }
        }
        if (n_hints) {
            upload(kind, kinds.data(), n_hints * 4);
            upload(in_off, h_in_off, (n_hints + 1) * 4);
            upload(expr_off, h_expr_off, (n_expr + 1) * 4);
            upload(term_wire, h_term_wire, n_terms * 4);
            upload(term_coeff, h_term_coeff, n_terms * 4);
            upload(out_start, h_out_start, n_hints * 4);
            upload(lvl_hints, h_level_hints, n_hints * 4);
            upload(lvl_pref, pf.data(), (n_hints + 1) * 4);
            packed.alloc(n_hints * 64);
        }
        level_off.assign(h_level_off, h_level_off + n_levels + 1);
        pref = std::move(pf);
        min_out = lowest;
        n = n_hints;
        set = true;
    }

    size_t launches() const {
        size_t nl = 0;
        for (size_t l = 0; l + 1 < level_off.size(); l++) {
            const uint32_t a = level_off[l], b = level_off[l + 1];
            if (b > a) nl += 1 + (pref[b] > pref[a]);
        }
        return nl;
    }

    // level l's hint launches on st (same stream, hence same captured chain, as
    // the level's constraint launch; they come first, so a hint never sees a
    // wire its own level's constraints solve)
    template <class C>
    void enqueue_level(size_t l, hipStream_t st, const Fe<C>* coef, uint32_t one_idx, Fe<C>* W, uint8_t* solved,
                       uint32_t* fail) const {
        if (!n) return;
        const uint32_t a = level_off[l], cnt = level_off[l + 1] - a;
        if (!cnt) return;
        HintDev<C> d{kind.as<uint32_t>(),       in_off.as<uint32_t>(),    expr_off.as<uint32_t>(),
                     term_wire.as<uint32_t>(),  term_coeff.as<uint32_t>(), out_start.as<uint32_t>(),
                     lvl_hints.as<uint32_t>(),  lvl_pref.as<uint32_t>(),  packed.as<uint32_t>(),
                     coef, one_idx, W, solved, fail};
        hipLaunchKernelGGL(k_hint_eval<C>, dim3(grid_for(cnt, 256)), dim3(256), 0, st, d, a, cnt);
        GG_HIP(hipGetLastError());
        const uint32_t n_out = pref[a + cnt] - pref[a];
        if (!n_out) return;
        hipLaunchKernelGGL(k_hint_scatter<C>, dim3(grid_for(n_out, 256)), dim3(256), 0, st, d, a, cnt, n_out);
        GG_HIP(hipGetLastError());
    }
};

// the hint's message for a fail[1] with HINT_FAIL_BIT set
inline std::string hint_unsolved_message(uint32_t f) {
    return "hint #" + std::to_string(f & ~HINT_FAIL_BIT) +
           ": input wire unsolved at its level (the levels do not match the system)";
}

// gg_hint_eval_host for one field
template <class C>
inline void hint_eval_host(uint32_t kind, const void* inputs, size_t n_in, void* outputs, size_t n_out) {
    const Fe<C>* in = (const Fe<C>*)inputs;
    Fe<C>* out = (Fe<C>*)outputs;
    uint32_t packed[16];
    hint_eval<C>(kind, in[0], n_in > 1 ? in[1] : Fe<C>::zero(), packed);
    for (size_t j = 0; j < n_out; j++) {
        if (hint_is_field(kind)) {
            for (int i = 0; i < 8; i++) out[j].v[i] = packed[i];
        } else {
            out[j] = hint_const<C>(hint_digit(kind, packed, (uint32_t)std::min<size_t>(j, 0xffffffffu)));
        }
    }
}

}  // namespace gg

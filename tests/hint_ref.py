"""TEST INFRASTRUCTURE ONLY (the checker of tests/test_hints_cpu.py and
tests/test_gpu_hints.py, never the product path): gnark's built-in hints and
the solver around them restated from the Go in Python big-int arithmetic.

    the seven hint functions, line by line:
        inv_zero          constraint/solver/hint_registry.go:77-90
        ith_bit, n_bits,
        n_trits, n_naf    std/math/bits/hints.go:26-114
        cmp_in_field,
        min_output,
        is_less_output    std/math/cmp/bounded.go:192-229
    solve_with_hints      constraint/bn254/solver.go level by level: a hint as
                          solveWithHint (solver.go:197-246), an R1C as
                          oracle/r1cs_solver.py:solve does
    solve_scs_with_hints  the same around oracle/scs_solver.py:solve's step
    levels_with_hints     r1cs.Levels of hints and constraints in instruction
                          order (blueprint_hint.go:75-106, blueprint_r1cs.go:61-96)
                          by a memoised producer walk, a different route from
                          the mirror's single pass
    random_circuit / random_scs_circuit
                          random systems with hints of all seven kinds interleaved

HintID = FNV-1a-32 of the Go function name (constraint/solver/hint.go:87-96);
the values are computed from that definition (no reference fixture pins them).
A hint here is H(hint_id, inputs, out_start, out_end, before): inputs are
linear expressions [(wire, coeff)], CONST_WIRE marks a constant term, before is
the index of the constraint the hint precedes in instruction order.
"""
from __future__ import annotations

from collections import namedtuple

H = namedtuple("H", "hint_id inputs out_start out_end before")
CONST_WIRE = 0xFFFFFFFF

INV_ZERO = 0x970C3C2F
ITH_BIT = 0xCC606925
N_BITS = 0xF54CDBEB
N_TRITS = 0x7F90A7AD
N_NAF = 0x5CA55EC0
MIN_OUTPUT = 0x7970DDA3
IS_LESS_OUTPUT = 0x73E09B3C

GO_NAMES = {
    INV_ZERO: "github.com/consensys/gnark/constraint/solver.InvZeroHint",
    ITH_BIT: "github.com/consensys/gnark/std/math/bits.ithBit",
    N_BITS: "github.com/consensys/gnark/std/math/bits.nBits",
    N_TRITS: "github.com/consensys/gnark/std/math/bits.nTrits",
    N_NAF: "github.com/consensys/gnark/std/math/bits.nNaf",
    MIN_OUTPUT: "github.com/consensys/gnark/std/math/cmp.minOutputHint",
    IS_LESS_OUTPUT: "github.com/consensys/gnark/std/math/cmp.isLessOutputHint",
}
ARITY = {INV_ZERO: (1, 1), ITH_BIT: (2, 1), N_BITS: (1, None), N_TRITS: (1, None), N_NAF: (1, None),
         MIN_OUTPUT: (2, 1), IS_LESS_OUTPUT: (2, 1)}  # inputs, outputs (None: any)


def _is_uint64(x):
    return 0 <= x < 1 << 64


def inv_zero(q, inputs, results):
    result = inputs[0]
    if _is_uint64(result) and result == 0:
        results[0] = result
        return
    results[0] = pow(result, -1, q)  # ModInverse


def ith_bit(q, inputs, results):
    if not _is_uint64(inputs[1]):
        results[0] = 0
        return
    # int(inputs[1].Uint64()) goes negative from 2^63 on and big.Int.Bit panics;
    # the GPU solver defines those indices as 0 (include/gnark_amd.h)
    i = inputs[1]
    results[0] = 0 if i >= 1 << 63 else (inputs[0] >> i) & 1


def n_bits(q, inputs, results):
    n = inputs[0]
    for i in range(len(results)):
        results[i] = (n >> i) & 1


def _text3(n):
    if n == 0:
        return "0"
    s = ""
    while n:
        s = chr(48 + n % 3) + s
        n //= 3
    return s


def n_trits(q, inputs, results):
    base3 = _text3(inputs[0])
    i = 0
    j = len(base3) - 1
    while j >= 0 and i < len(results):
        results[i] = ord(base3[j]) - 48
        i += 1
        j -= 1
    while i < len(results):
        results[i] = 0
        i += 1


def n_naf(q, inputs, results):
    a = inputs[0]
    n = 0
    while a != 0 and n < len(results):
        if a & 1 == 0:
            results[n] = 0
        elif a & 3 == 3:
            results[n] = -1
            a += 1
        else:
            results[n] = 1
        a >>= 1
        n += 1
    while n < len(results):
        results[n] = 0
        n += 1


def _cmp(a, b):
    return (a > b) - (a < b)


def cmp_in_field(a, b, order):
    biggest_positive = order >> 1
    if _cmp(a, biggest_positive) * _cmp(b, biggest_positive) == -1:
        return -_cmp(a, b)
    return _cmp(a, b)


def min_output(q, inputs, results):
    a, b = inputs
    results[0] = a if cmp_in_field(a, b, q) == -1 else b


def is_less_output(q, inputs, results):
    a, b = inputs
    results[0] = 1 if cmp_in_field(a, b, q) == -1 else 0


HINTS = {INV_ZERO: inv_zero, ITH_BIT: ith_bit, N_BITS: n_bits, N_TRITS: n_trits, N_NAF: n_naf,
         MIN_OUTPUT: min_output, IS_LESS_OUTPUT: is_less_output}


def eval_hint(q, hint_id, inputs, n_out):
    """f(q, inputs, outputs) then fr.SetBigInt of every output (solver.go:230-237)."""
    results = [0] * n_out
    HINTS[hint_id](q, [int(x) for x in inputs], results)
    return [r % q for r in results]


# ---- levels ----------------------------------------------------------------

def _instructions(n_constraints, hints):
    at = [[] for _ in range(n_constraints + 1)]
    for i, h in enumerate(hints):
        at[h.before].append(i)
    out = []
    for c in range(n_constraints + 1):
        out += [("h", i) for i in at[c]]
        if c < n_constraints:
            out.append(("c", c))
    return out


def levels_with_hints(nb_inputs, cons_wires, hints):
    """cons_wires[c]: the wires constraint c mentions.  Returns (constraint
    levels, hint levels), two lists of the same length."""
    ins = _instructions(len(cons_wires), hints)
    producer = {}
    for idx, (kind, i) in enumerate(ins):
        ws = range(hints[i].out_start, hints[i].out_end) if kind == "h" else cons_wires[i]
        for w in ws:
            if w != CONST_WIRE and w >= nb_inputs and w not in producer:
                producer[w] = idx
    lvl = {}

    def level(idx):
        if idx in lvl:
            return lvl[idx]
        kind, i = ins[idx]
        if kind == "h":
            reads = [w for e in hints[i].inputs for w, _ in e]
        else:
            reads = cons_wires[i]
        # a wire placed only later in instruction order has no level yet when
        # this instruction is placed (LevelUnset): it does not count
        deps = [producer[w] for w in reads
                if w != CONST_WIRE and w >= nb_inputs and w in producer and producer[w] < idx]
        lvl[idx] = 1 + max((level(d) for d in deps), default=-1)
        return lvl[idx]

    cl, hl = [], []
    for idx, (kind, i) in enumerate(ins):
        lv = level(idx)
        while len(cl) <= lv:
            cl.append([])
            hl.append([])
        (hl if kind == "h" else cl)[lv].append(i)
    return cl, hl


def r1cs_wires(constraints):
    return [[w for side in k for w, _ in side] for k in constraints]


def scs_wires(cons):
    return [list(k[:3]) for k in cons]


# ---- solvers ---------------------------------------------------------------

class Unsatisfied(Exception):
    def __init__(self, cid, why):
        super().__init__("constraint #%d: %s" % (cid, why))
        self.cid = cid


class HintUnsolved(Exception):
    def __init__(self, hid):
        super().__init__("hint #%d: input wire unsolved at its level" % hid)
        self.hid = hid


def _solve_hint(mod, W, solved, k, h):
    inputs = []
    for e in h.inputs:
        v = 0
        for w, c in e:
            if w == CONST_WIRE:
                v += c
                continue
            if not solved[w]:
                raise HintUnsolved(k)
            v += c * W[w]
        inputs.append(v % mod)
    outs = eval_hint(mod, h.hint_id, inputs, h.out_end - h.out_start)
    for j, v in enumerate(outs):
        W[h.out_start + j] = v
        solved[h.out_start + j] = True


def solve_with_hints(mod, nb_wires, constraints, hints, witness, levels):
    """R1CS: witness = the values after ONE_WIRE; levels = (constraint levels,
    hint levels).  Returns (W, A, B, C) or raises Unsatisfied(cid)."""
    inv = lambda x: pow(x, mod - 2, mod)
    W = [0] * nb_wires
    solved = [False] * nb_wires
    W[0], solved[0] = 1, True
    for i, v in enumerate(witness):
        W[1 + i], solved[1 + i] = v % mod, True
    n = len(constraints)
    A, B, C = [0] * n, [0] * n, [0] * n
    for cl, hl in zip(*levels):
        for k in hl:
            _solve_hint(mod, W, solved, k, hints[k])
        for c in cl:
            acc = [0, 0, 0]
            unknown = None
            for s, side in enumerate(constraints[c]):
                for w, k in side:
                    if solved[w]:
                        acc[s] = (acc[s] + k * W[w]) % mod
                    elif unknown is not None:
                        raise Unsatisfied(c, "more than one wire to instantiate")
                    else:
                        unknown = (s, w, k % mod)
            a, b, cc = acc
            if unknown is None:
                if a * b % mod != cc:
                    raise Unsatisfied(c, "a b != c")
            else:
                s, w, k = unknown
                v = 0
                if s == 0:
                    if b:
                        v = (cc * inv(b) - a) % mod
                        acc[0] = (a + v) % mod
                    elif a * b % mod != cc:
                        raise Unsatisfied(c, "a b != c")
                elif s == 1:
                    if a:
                        v = (cc * inv(a) - b) % mod
                        acc[1] = (b + v) % mod
                    elif a * b % mod != cc:
                        raise Unsatisfied(c, "a b != c")
                else:
                    v = (a * b - cc) % mod
                    acc[2] = (cc + v) % mod
                W[w] = v * inv(k) % mod
                solved[w] = True
            A[c], B[c], C[c] = acc
    if not all(solved):
        raise Unsatisfied(-1, "solver didn't assign a value to all wires")
    return W, A, B, C


def solve_scs_with_hints(mod, n_wires, cons, hints, witness, levels):
    """Sparse R1CS: cons[c] = (xa, xb, xc, qL, qR, qO, qM, qC), witness at wires 0..; returns W."""
    inv = lambda x: pow(x, mod - 2, mod)
    W = [0] * n_wires
    solved = [False] * n_wires
    for i, v in enumerate(witness):
        W[i], solved[i] = v % mod, True
    for cl, hl in zip(*levels):
        for k in hl:
            _solve_hint(mod, W, solved, k, hints[k])
        for c in cl:
            xa, xb, xc, qL, qR, qO, qM, qC = cons[c]
            sa, sb, sc = solved[xa], solved[xb], solved[xc]
            if (not sa) + (not sb) + (not sc) > 1 or (not sa and xa == xb):
                raise Unsatisfied(c, "more than one unsolved wire")
            a, b, o = W[xa], W[xb], W[xc]
            if not sa or not sb:
                den = (qM * b + qL) % mod if not sa else (qM * a + qR) % mod
                if den == 0:
                    raise Unsatisfied(c, "division by zero")
                num = ((qR * b) if not sa else (qL * a)) + qO * o + qC
                w = xa if not sa else xb
                W[w] = (-num * inv(den)) % mod
                solved[w] = True
            elif not sc:
                if qO % mod == 0:
                    raise Unsatisfied(c, "division by zero")
                t = qM * a * b + qL * a + qR * b + qC
                W[xc] = (-t * inv(qO % mod)) % mod
                solved[xc] = True
            elif (qM * a * b + qL * a + qR * b + qO * o + qC) % mod:
                raise Unsatisfied(c, "not satisfied")
    if not all(solved):
        raise Unsatisfied(-1, "solver didn't assign a value to all wires")
    return W


# ---- random systems --------------------------------------------------------

KINDS = (INV_ZERO, ITH_BIT, N_BITS, N_TRITS, N_NAF, MIN_OUTPUT, IS_LESS_OUTPUT)


def _random_expr(rng, mod, known, const_wire):
    """A linear expression over solved wires: empty, a constant, unit and random coefficients."""
    r = rng.random()
    if r < 0.05:
        return []
    e = []
    for _ in range(rng.randrange(1, 4)):
        k = 1 if rng.random() < 0.3 else rng.randrange(1, mod)
        e.append((rng.choice(known), k))
    if rng.random() < 0.3:
        # a small constant keeps some values small (digits then end early)
        e.append((const_wire, rng.randrange(1, 1 << 20)))
    if rng.random() < 0.15:  # a small value on its own: a short digit expansion
        return [(const_wire, rng.randrange(0, 1 << 40))]
    return e


def _random_hint(rng, mod, known, nxt, budget, before, const_wire, index):
    kind = KINDS[index % len(KINDS)]  # every kind in turn
    n_in, n_out = ARITY[kind]
    if n_out is None:
        n_out = min(budget, rng.choice((1, 2, 7, 33)))
    inputs = [_random_expr(rng, mod, known, const_wire) for _ in range(n_in)]
    if kind == ITH_BIT:  # a bit index in range most of the time
        if rng.random() < 0.8:
            inputs[1] = [(const_wire, rng.randrange(0, 260))]
    if kind in (MIN_OUTPUT, IS_LESS_OUTPUT) and rng.random() < 0.2:
        inputs[1] = list(inputs[0])  # equal pair
    return H(kind, inputs, nxt, nxt + n_out, before)


def random_circuit(rng, mod, nb_public, nb_secret, n_internal, zero_divisor=False):
    """An R1CS as oracle/r1cs_solver.py:random_circuit builds it, with hints of
    all seven kinds interleaved; returns (constraints, hints, n_wires).  Wire 0
    (ONE_WIRE) carries the constants of the hint inputs."""
    nin = nb_public + nb_secret
    cons, hints = [], []
    known = list(range(nin))  # what a hint may read: every solved wire
    dense = list(range(nin))  # witness and constraint wires: random values, never 0 by construction
    hint_out = []             # hint outputs: mostly 0 and 1
    nxt = nin
    end = nin + n_internal
    while nxt < end:
        if rng.random() < 0.3:
            h = _random_hint(rng, mod, known, nxt, end - nxt, len(cons), 0, len(hints))
            hints.append(h)
            known += range(h.out_start, h.out_end)
            hint_out += range(h.out_start, h.out_end)
            nxt = h.out_end
            continue
        new = nxt
        nxt += 1
        sides = [[], [], []]
        for s in range(3):
            for _ in range(rng.randrange(1, 3)):
                sides[s].append((rng.choice(dense), rng.randrange(1, mod)))
            # a hint output joins a side that a dense term keeps away from zero
            # (a zero side would make the new wire's divisor vanish)
            if hint_out and rng.random() < 0.5:
                sides[s].append((rng.choice(hint_out), rng.randrange(1, mod)))
        tgt = rng.randrange(3)
        sides[tgt].append((new, rng.randrange(1, mod)))
        zero = zero_divisor and tgt < 2 and rng.random() < 0.3
        if zero:
            sides[1 - tgt] = [(0, 0)]
            sides[2] = [(0, 0)]
        cons.append(tuple(sides))
        if not zero:
            known.append(new)
            dense.append(new)
    return cons, hints, end


def random_scs_circuit(rng, mod, nb_public, nb_secret, n_internal):
    """A sparse R1CS in the shape of oracle/scs_solver.py:random_circuit (one new
    wire per constraint at xa, xb or xc) with hints interleaved; returns
    (cons, hints, n_wires).  Constants of hint inputs use CONST_WIRE."""
    nin = nb_public + nb_secret
    cons, hints = [], []
    known = list(range(nin))
    nxt = nin
    end = nin + n_internal
    while nxt < end:
        if rng.random() < 0.3:
            h = _random_hint(rng, mod, known, nxt, end - nxt, len(cons), CONST_WIRE, len(hints))
            hints.append(h)
            known += range(h.out_start, h.out_end)
            nxt = h.out_end
            continue
        r = rng.random()
        x, y = rng.choice(known), rng.choice(known)
        if r < 0.3:
            cons.append((x, y, nxt, 0, 0, mod - 1, rng.randrange(1, mod), 0))
        elif r < 0.55:
            cons.append((x, y, nxt, rng.randrange(mod), rng.randrange(mod), mod - 1, 0, rng.randrange(mod)))
        elif r < 0.8:
            cons.append((nxt, y, x, rng.randrange(1, mod), rng.randrange(mod), rng.randrange(mod),
                         rng.randrange(mod), rng.randrange(mod)))
        else:
            cons.append((x, nxt, y, rng.randrange(mod), rng.randrange(1, mod), rng.randrange(mod),
                         rng.randrange(mod), rng.randrange(mod)))
        known.append(nxt)
        nxt += 1
    return cons, hints, end

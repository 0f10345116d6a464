"""R1CS solver on MI355X: mirror of cs.R1CS's Solve (constraint/bn254/
solver.go:418-608, system.go:64-104), the system resident in HBM and the
solution left there for the prover.  Hint calls: gnark's own seven hints
(HINT_IDS) run on the GPU, passed as ``hints=[Hint(...)]``; any other hint is
refused (such systems keep gnark's host solver).

    sys = R1CS.from_terms(nb_public, nb_secret, n_wires, constraints)   # once
    sol = sys.solve(witness_values)            # -> groth16.Solution (on device)
    proof = groth16.prove(pk, sol, with_amd_acceleration())

``constraints`` are (L, R, O) lists of (wire, coefficient) pairs, the terms
r1cs.GetR1Cs() yields; the coefficient table and the CSR arrays are built here
(r1cs.Coefficients), and the levels are r1cs.Levels as gnark's level builder
assigns them (constraint/blueprint_r1cs.go:61-96: an R1C sits one level above
the deepest internal wire it reads and places its unsolved wires there)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import fr
from ._lib import check, lib, ptr, DeviceBuffer

GG_ERR_UNSATISFIED = 6


class UnsatisfiedConstraintError(RuntimeError):
    """solver.UnsatisfiedConstraintError (solver.go:610-623)."""

    def __init__(self, cid: int, msg: str):
        super().__init__(msg)
        self.cid = cid


_GNARK = "github.com/consensys/gnark/"
HINT_NAMES = (
    _GNARK + "constraint/solver.InvZeroHint",
    _GNARK + "std/math/bits.ithBit",
    _GNARK + "std/math/bits.nBits",
    _GNARK + "std/math/bits.nTrits",
    _GNARK + "std/math/bits.nNaf",
    _GNARK + "std/math/cmp.minOutputHint",
    _GNARK + "std/math/cmp.isLessOutputHint",
)


def hint_id(go_name: str) -> int:
    """solver.GetHintID: FNV-1a-32 of the Go function name (constraint/solver/hint.go:87-96)."""
    h = 0x811C9DC5
    for c in go_name.encode():
        h = ((h ^ c) * 0x01000193) & 0xFFFFFFFF
    return h


# the hints the GPU solvers evaluate (gg_hint_supported), name -> HintID
HINT_IDS = {name: hint_id(name) for name in HINT_NAMES}


@dataclass
class Hint:
    """One hint instruction (constraint.HintMapping): ``inputs`` are linear
    expressions [(wire, coeff int), ...] (a constant: (0, k) in an R1CS, whose
    wire 0 is ONE_WIRE, or (CONST_WIRE, k) in either system), the outputs are
    wires out_start .. out_end - 1, and ``before`` is the index of the constraint
    it precedes in instruction order (len(constraints): after the last one)."""
    hint_id: int
    inputs: list
    out_start: int
    out_end: int
    before: int


CONST_WIRE = 0xFFFFFFFF  # a constant term of a hint input (Term.IsConstant)


def hint_supported(hid: int):
    """(supported, Go name or None) of gg_hint_supported."""
    ok, name = ctypes.c_int(), ctypes.c_char_p()
    check(lib.gg_hint_supported(hid, ctypes.byref(ok), ctypes.byref(name)))
    return bool(ok.value), name.value.decode() if name.value else None


def hint_eval_host(curve: str, hid: int, inputs: Sequence[int], n_out: int) -> list:
    """One hint on the CPU by the library's own arithmetic (gg_hint_eval_host):
    inputs and the returned outputs are integers in [0, r)."""
    from ._lib import GG_CURVE_BN254, GG_CURVE_BLS12_381
    bn = curve == "bn254"
    mont, unmont, mod = (fr.fr_mont, fr.fr_unmont, fr.R) if bn else (fr.bls_fr_mont, fr.bls_fr_unmont, fr.BLS_R)
    ibuf = b"".join(mont(int(v) % mod) for v in inputs) or bytes(32)
    obuf = bytearray(32 * max(n_out, 1))
    check(lib.gg_hint_eval_host(GG_CURVE_BN254 if bn else GG_CURVE_BLS12_381, hid, ptr(ibuf), len(inputs),
                                ptr(obuf), n_out))
    return [unmont(bytes(obuf[32 * i:32 * i + 32])) for i in range(n_out)]


def _hint_order(hints, n_constraints):
    """Instruction order: ("h", i) / ("c", j), hint i just before constraint hints[i].before."""
    at = {}
    for i, h in enumerate(hints):
        if not 0 <= h.before <= n_constraints:
            raise ValueError("hint %d: before=%d outside [0, %d]" % (i, h.before, n_constraints))
        at.setdefault(h.before, []).append(i)
    for c in range(n_constraints + 1):
        for i in at.get(c, ()):
            yield "h", i
        if c < n_constraints:
            yield "c", c


def _place_hint(level, nb_inputs, h):
    """BlueprintGenericHint.UpdateInstructionTree (blueprint_hint.go:75-106): the
    outputs sit one level above the deepest input wire."""
    mx = -1
    for expr in h.inputs:
        for w, _ in expr:
            if w == CONST_WIRE or w < nb_inputs:
                continue
            if level[w] > mx:
                mx = int(level[w])
    mx += 1
    level[h.out_start:h.out_end] = mx
    return mx


def _levels_with_hints(nb_inputs, n_wires, n_constraints, hints, cons_wires):
    level = np.full(n_wires, -1, dtype=np.int64)
    cl, hl = [], []
    for kind, i in _hint_order(hints, n_constraints):
        if kind == "h":
            mx, dst = _place_hint(level, nb_inputs, hints[i]), hl
        else:
            mx, outs, dst = -1, [], cl
            for w in cons_wires(i):
                w = int(w)
                if w < nb_inputs:
                    continue
                if level[w] < 0:
                    if w not in outs:
                        outs.append(w)
                elif level[w] > mx:
                    mx = int(level[w])
            mx += 1
            for w in outs:
                level[w] = mx
        while len(cl) <= mx:
            cl.append([])
            hl.append([])
        dst[mx].append(i)
    return cl, hl


def compute_levels_with_hints(nb_inputs: int, n_wires: int, term_off, term_wire, hints) -> tuple:
    """r1cs.Levels of a system with hint instructions, split into the constraints
    and the hints of each level (two lists of the same length): hints and R1Cs
    walked in instruction order (blueprint_hint.go:75-106, blueprint_r1cs.go:61-96)."""
    ncons = (len(term_off) - 1) // 3
    return _levels_with_hints(nb_inputs, n_wires, ncons, hints,
                              lambda c: term_wire[int(term_off[3 * c]):int(term_off[3 * c + 3])])


def compute_scs_levels_with_hints(nb_inputs: int, n_wires: int, wires, hints) -> tuple:
    """compute_levels_with_hints for a sparse R1CS (xa, xb, xc per constraint)."""
    w = np.asarray(wires, dtype=np.int64).reshape(-1, 3)
    return _levels_with_hints(nb_inputs, n_wires, len(w), hints, lambda c: w[c])


def _hint_arrays(hints, hint_levels, coeff_index):
    """The gg_*_set_hints arrays; coeff_index(k) -> index into the handle's table."""
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
    ids, in_off, expr_off, tw, tc, o0, o1 = [], [0], [0], [], [], [], []
    for h in hints:
        ids.append(h.hint_id)
        for expr in h.inputs:
            for w, k in expr:
                tw.append(w)
                tc.append(coeff_index(k))
            expr_off.append(len(tw))
        in_off.append(len(expr_off) - 1)
        o0.append(h.out_start)
        o1.append(h.out_end)
    lo = np.zeros(len(hint_levels) + 1, dtype=np.uint32)
    lo[1:] = np.cumsum([len(x) for x in hint_levels])
    lh = [i for lv in hint_levels for i in lv]
    return [u32(a) for a in (ids, in_off, expr_off, tw, tc, o0, o1, lo, lh)], len(hint_levels)


def compute_levels(nb_inputs: int, n_wires: int, term_off, term_wire) -> list:
    """r1cs.Levels from the CSR terms (blueprint_r1cs.go:61-96, core.go:405-419):
    wires < nb_inputs are inputs (not in the instruction tree)."""
    return compute_levels_with_hints(nb_inputs, n_wires, term_off, term_wire, ())[0]


def compute_scs_levels(nb_inputs: int, n_wires: int, wires) -> list:
    """r1cs.Levels of a sparse R1CS (blueprint.go updateInstructionTree over
    xa, xb, xc): wires < nb_inputs are the witness."""
    return compute_scs_levels_with_hints(nb_inputs, n_wires, wires, ())[0]


def _intern(table, index, k):
    """Index of coefficient k in table, appended when new (r1cs.Coefficients)."""
    if k not in index:
        index[k] = len(table)
        table.append(k)
    return index[k]


class _System:
    """What R1CS and SparseR1CS share: the scalar field, the levels and the
    coefficient table as the library takes them, the hints, and the handle's
    schedule / release / error mapping.  A subclass names its C functions."""
    _set_hints_fn = _schedule_fn = _release_fn = None

    def _field(self, curve, bn254):
        """Sets curve, mod and the Montgomery conversion; returns the GG_CURVE_* id."""
        from ._lib import GG_CURVE_BN254, GG_CURVE_BLS12_381
        self.curve = curve
        self.mod = fr.R if bn254 else fr.BLS_R
        self._mont = fr.fr_mont if bn254 else fr.bls_fr_mont
        return GG_CURVE_BN254 if bn254 else GG_CURVE_BLS12_381

    def _set_levels(self, hints, levels, hint_levels, compute):
        """self.hints / levels / hint_levels; compute(hints) -> (levels, hint_levels)
        fills in what the caller left out.  Returns the levels flattened:
        (level_off, level_cons) of gg_*_create."""
        self.hints = list(hints) if hints else None
        if self.hints and (levels is None or hint_levels is None):
            levels, hint_levels = compute(self.hints)
        if levels is None:
            levels = compute(())[0]
        self.levels, self.hint_levels = levels, hint_levels
        lo = np.zeros(len(levels) + 1, dtype=np.uint32)
        lo[1:] = np.cumsum([len(x) for x in levels])
        lc = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in levels])
                                  if levels else np.zeros(0, dtype=np.uint32), dtype=np.uint32)
        return lo, lc

    def _coeff_bytes(self, coeffs):
        return b"".join(self._mont(int(k) % self.mod) for k in coeffs)

    def _set_own_hints(self, coeffs):
        if self.hints:
            index = {int(k) % self.mod: i for i, k in reversed(list(enumerate(coeffs)))}
            self.set_hints(self.hints, self.hint_levels, lambda k: index[int(k) % self.mod])

    def set_hints(self, hints, hint_levels, coeff_index):
        """gg_*_set_hints: once, before the first solve."""
        arrs, n_levels = _hint_arrays(hints, hint_levels, coeff_index)
        check(self._set_hints_fn(self.handle, len(hints), *(ptr(a) for a in arrs), n_levels))

    def schedule(self):
        """(strands, launches, segments) of the last solve (gg_*_schedule)."""
        s, nl, ns = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        check(self._schedule_fn(self.handle, ctypes.byref(s), ctypes.byref(nl), ctypes.byref(ns)))
        return bool(s.value), nl.value, ns.value

    @staticmethod
    def _raise_for(rc, bad):
        if rc == GG_ERR_UNSATISFIED:
            raise UnsatisfiedConstraintError(bad.value, lib.gg_last_error().decode())
        check(rc)

    def close(self):
        if getattr(self, "handle", None):
            self._release_fn(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class R1CS(_System):
    """Device-resident R1CS (gg_r1cs_create) with its solver."""
    _set_hints_fn, _schedule_fn, _release_fn = lib.gg_r1cs_set_hints, lib.gg_r1cs_schedule, lib.gg_r1cs_release

    def __init__(self, nb_public: int, nb_secret: int, n_wires: int, term_off, term_wire, term_coeff,
                 coeffs: Sequence[int], levels: Optional[Sequence[Sequence[int]]] = None,
                 curve: str = "bn254", hints=None, hint_levels=None):
        cid = self._field(curve, curve == "bn254")
        self.nb_public, self.nb_secret, self.n_wires = nb_public, nb_secret, n_wires
        self.term_off = np.ascontiguousarray(term_off, dtype=np.uint32)
        self.term_wire = np.ascontiguousarray(term_wire, dtype=np.uint32)
        self.term_coeff = np.ascontiguousarray(term_coeff, dtype=np.uint32)
        self.n_constraints = (len(self.term_off) - 1) // 3
        lo, lc = self._set_levels(hints, levels, hint_levels, lambda hs: compute_levels_with_hints(
            nb_public + nb_secret, n_wires, self.term_off, self.term_wire, hs))
        cbytes = self._coeff_bytes(coeffs)
        h = ctypes.c_void_p()
        check(lib.gg_r1cs_create_ex(cid, n_wires, self.n_constraints, ptr(self.term_off), ptr(self.term_wire),
                                    ptr(self.term_coeff), ptr(cbytes), len(coeffs), ptr(lo), ptr(lc),
                                    len(self.levels), ctypes.byref(h)))
        self.handle = h
        # newSolver's witness-size check, enforced by the library too (solver.go:71-76)
        check(lib.gg_r1cs_set_inputs(h, nb_public, nb_secret))
        self._set_own_hints(coeffs)

    @classmethod
    def from_terms(cls, nb_public: int, nb_secret: int, n_wires: int, constraints, levels=None,
                   curve: str = "bn254", hints=None, hint_levels=None) -> "R1CS":
        """constraints: [(L, R, O)] with L = [(wire, coeff int), ...]; hints: [Hint]
        (their coefficients join the same table; levels / hint_levels default to
        compute_levels_with_hints)."""
        mod = fr.R if curve == "bn254" else fr.BLS_R
        table, index = [], {}
        off, wires, cids = [0], [], []
        for L, R, O in constraints:
            for side in (L, R, O):
                for w, k in side:
                    wires.append(w)
                    cids.append(_intern(table, index, k % mod))
                off.append(len(wires))
        for h in hints or ():
            for expr in h.inputs:
                for _, k in expr:
                    _intern(table, index, k % mod)
        if not table:
            table = [1]
        return cls(nb_public, nb_secret, n_wires, off, wires, cids, table, levels, curve, hints, hint_levels)

    def info(self):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib.gg_r1cs_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def solve(self, witness, on_device: bool = True):
        """r1cs.Solve(fullWitness): witness = public (without ONE_WIRE) then
        secret values (ints, or Montgomery bytes / a DeviceBuffer).  Returns a
        groth16.Solution whose W, A, B, C live in HBM (on_device) or on the host."""
        from .groth16 import Solution
        n_in = self.nb_public - 1 + self.nb_secret
        wdev = False
        if isinstance(witness, DeviceBuffer):
            wbuf, wdev = witness, True
        elif isinstance(witness, (bytes, bytearray)):
            wbuf = bytes(witness)
        else:
            wbuf = b"".join(self._mont(int(v) % self.mod) for v in witness)
            if len(witness) != n_in:
                raise ValueError("invalid witness size, got %d, expected %d" % (len(witness), n_in))
        if not wdev and len(wbuf) != 32 * n_in:
            raise ValueError("invalid witness size, got %d bytes, expected %d" % (len(wbuf), 32 * n_in))
        nw, nc = self.n_wires, self.n_constraints
        if on_device:
            W, A, B, C = (DeviceBuffer(max(32 * k, 32)) for k in (nw, nc, nc, nc))
        else:
            W, A, B, C = (bytearray(32 * k) for k in (nw, nc, nc, nc))
        bad = ctypes.c_int64(-1)
        rc = lib.gg_r1cs_solve(self.handle, ptr(wbuf), n_in, int(wdev), ptr(W), ptr(A), ptr(B), ptr(C),
                               int(on_device), ctypes.byref(bad))
        self._raise_for(rc, bad)
        return Solution(W, A, B, C, nw, nc, on_device=on_device)

    def solve_resident(self, witness: bytes):
        """solve() without copies: the returned Solution points at the handle's own
        HBM buffers (valid until the next solve or close) -- the shape a prover
        pipeline uses (witness in, proof out, the solution never leaves HBM)."""
        from .groth16 import Solution
        n_in = self.nb_public - 1 + self.nb_secret
        if len(witness) != 32 * n_in:
            raise ValueError("invalid witness size, got %d bytes, expected %d" % (len(witness), 32 * n_in))
        bad = ctypes.c_int64(-1)
        rc = lib.gg_r1cs_solve(self.handle, ptr(witness), n_in, 0, None, None, None, None, 1, ctypes.byref(bad))
        self._raise_for(rc, bad)
        p = [ctypes.c_void_p() for _ in range(4)]
        check(lib.gg_r1cs_solution_dev(self.handle, *(ctypes.byref(x) for x in p)))
        return Solution(p[0], p[1], p[2], p[3], self.n_wires, self.n_constraints, on_device=True)


class SparseR1CS(_System):
    """Device-resident sparse R1CS (gg_scs_create) with its solver: the PlonK
    side of r1cs.Solve (constraint/blueprint_scs.go:53-151), returning the
    L, R, O columns of evaluateLROSmallDomain (system.go:221-264)."""
    _set_hints_fn, _schedule_fn, _release_fn = lib.gg_scs_set_hints, lib.gg_scs_schedule, lib.gg_scs_release

    def __init__(self, nb_public: int, nb_secret: int, n_wires: int, wires, qidx, coeffs: Sequence[int],
                 flags=None, levels=None, curve: str = "bls12-381", hints=None, hint_levels=None):
        cid = self._field(curve, curve != "bls12-381")
        self.nb_public, self.nb_secret, self.n_wires = nb_public, nb_secret, n_wires
        self.wires = np.ascontiguousarray(wires, dtype=np.uint32)
        self.qidx = np.ascontiguousarray(qidx, dtype=np.uint32)
        self.n_constraints = len(self.wires) // 3
        self.flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        lo, lc = self._set_levels(hints, levels, hint_levels, lambda hs: compute_scs_levels_with_hints(
            nb_public + nb_secret, n_wires, self.wires, hs))
        cbytes = self._coeff_bytes(coeffs)
        self.coeffs_mont = cbytes  # the coefficient table as uploaded (plonk_prover.setup reads it)
        h = ctypes.c_void_p()
        check(lib.gg_scs_create(cid, n_wires, self.n_constraints, nb_public, ptr(self.wires), ptr(self.qidx),
                                ptr(self.flags), ptr(cbytes), len(coeffs), ptr(lo), ptr(lc),
                                len(self.levels), ctypes.byref(h)))
        self.handle = h
        check(lib.gg_scs_set_inputs(h, nb_public, nb_secret))
        self._set_own_hints(coeffs)
        d = ctypes.c_size_t()
        check(lib.gg_scs_info(h, None, None, ctypes.byref(d)))
        self.domain = d.value

    @classmethod
    def from_constraints(cls, nb_public: int, nb_secret: int, n_wires: int, constraints, flags=None,
                         levels=None, curve: str = "bls12-381", hints=None, hint_levels=None) -> "SparseR1CS":
        """constraints: [(xa, xb, xc, qL, qR, qO, qM, qC)] with int coefficients;
        hints: [Hint] (no ONE_WIRE here: a constant term is (CONST_WIRE, k))."""
        mod = fr.BLS_R if curve == "bls12-381" else fr.R
        table, index = [0, 1], {0: 0, 1: 1}
        wires, qidx = [], []
        for xa, xb, xc, *qs in constraints:
            wires += [xa, xb, xc]
            qidx += [_intern(table, index, k % mod) for k in qs]
        for h in hints or ():
            for expr in h.inputs:
                for _, k in expr:
                    _intern(table, index, k % mod)
        return cls(nb_public, nb_secret, n_wires, wires, qidx, table, flags, levels, curve, hints, hint_levels)

    def solve(self, witness, on_device: bool = True):
        """spr.Solve(fullWitness) -> (W, L, R, O): host bytes or DeviceBuffers."""
        n_in = self.nb_public + self.nb_secret
        if len(witness) != n_in:
            raise ValueError("invalid witness size, got %d, expected %d" % (len(witness), n_in))
        wbuf = b"".join(self._mont(int(v) % self.mod) for v in witness)
        nw, d = self.n_wires, self.domain
        if on_device:
            out = [DeviceBuffer(32 * nw), DeviceBuffer(32 * d), DeviceBuffer(32 * d), DeviceBuffer(32 * d)]
        else:
            out = [bytearray(32 * nw), bytearray(32 * d), bytearray(32 * d), bytearray(32 * d)]
        bad = ctypes.c_int64(-1)
        rc = lib.gg_scs_solve(self.handle, ptr(wbuf), n_in, 0, *(ptr(x) for x in out), int(on_device),
                              ctypes.byref(bad))
        self._raise_for(rc, bad)
        return out

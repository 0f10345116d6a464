"""gnark's built-in hints inside the GPU solvers (gg_r1cs_set_hints /
gg_scs_set_hints, csrc/hints.cuh) against the from-spec restatement
tests/hint_ref.py: wires and A, B, C (or L, R, O) bit-exact on the gadgets the
frontend emits (IsZero, ToBinary), on the block / wave boundaries of the two
hint kernels, on every form of input expression, on random circuits with all
seven hints interleaved (R1CS and sparse R1CS, both scalar fields), the error
paths, and a Groth16 proof from a solution the GPU solved with hints."""
import random

import pytest

import bn254_oracle as o
import hint_ref as hr
import scs_solver as sc

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_UNSUPPORTED = 1, 4
CURVES = ["bn254", "bls12-381"]


def _mod(curve):
    from gnark_amd import fr
    return fr.R if curve == "bn254" else fr.BLS_R


def _vals(buf, curve):
    from gnark_amd import fr
    un = fr.fr_unmont if curve == "bn254" else fr.bls_fr_unmont
    buf = bytes(buf)
    return [un(buf[i:i + 32]) for i in range(0, len(buf), 32)]


def _hints(hs):
    from gnark_amd import solver
    return [solver.Hint(*h) for h in hs]


def _solve_r1cs(sys_, wit, ncons):
    sol = sys_.solve(wit)
    out = [_vals(x.to_host(), sys_.curve) for x in (sol.W, sol.A, sol.B, sol.C)]
    return [out[0]] + [x[:ncons] for x in out[1:]]


def _check_r1cs(curve, nbp, nbs, nw, cons, hints, witnesses):
    """Build the handle, solve every witness, compare with hint_ref; returns the handle."""
    from gnark_amd import solver
    mod = _mod(curve)
    lv = hr.levels_with_hints(nbp + nbs, hr.r1cs_wires(cons), hints)
    sys_ = solver.R1CS.from_terms(nbp, nbs, nw, cons, curve=curve, hints=_hints(hints))
    for wit in witnesses:
        want = hr.solve_with_hints(mod, nw, cons, hints, wit, lv)
        got = _solve_r1cs(sys_, wit, len(cons))
        for name, g, w in zip("WABC", got, want):
            assert g == list(w), name
        assert sys_.schedule()[0] is False  # a handle with hints runs the level schedule
    return sys_


# ------------------------------------------------------------------ gadgets
def _is_zero_circuit(mod):
    # wires: 0 ONE, 1 a (secret), 2 m, 3 x = InvZero(a)   (api.go:547-564)
    cons = [([(1, mod - 1)], [(3, 1)], [(2, 1), (0, mod - 1)]),   # (-a) x = m - 1
            ([(1, 1)], [(2, 1)], [(0, 0)])]                       # a m = 0
    return cons, [hr.H(hr.INV_ZERO, [[(1, 1)]], 3, 4, 0)]


@pytest.mark.parametrize("curve", CURVES)
def test_is_zero(curve):
    mod = _mod(curve)
    cons, hints = _is_zero_circuit(mod)
    sys_ = _check_r1cs(curve, 1, 1, 4, cons, hints, [[0], [1], [mod - 1], [0x1234567890ABCDEF << 100]])
    W = _solve_r1cs(sys_, [0], 2)[0]
    assert W[2] == 1 and W[3] == 0          # m = 1, x = 0 for a = 0
    W = _solve_r1cs(sys_, [7], 2)[0]
    assert W[2] == 0 and W[3] * 7 % mod == 1
    sys_.close()


def _to_binary_circuit(mod, nbits):
    # wires: 0 ONE, 1 y (public claim), 2 x (secret), 3.. bits of x
    cons = [([(3 + i, 1)], [(0, 1), (3 + i, mod - 1)], [(0, 0)]) for i in range(nbits)]  # b (1 - b) = 0
    cons.append(([(3 + i, 1 << i) for i in range(nbits)], [(0, 1)], [(1, 1)]))           # sum 2^i b_i = y
    return cons, [hr.H(hr.N_BITS, [[(2, 1)]], 3, 3 + nbits, 0)]


@pytest.mark.parametrize("curve", CURVES)
def test_to_binary(curve):
    from gnark_amd import solver
    mod = _mod(curve)
    nbits = 254 if curve == "bn254" else 255
    cons, hints = _to_binary_circuit(mod, nbits)
    rnd = random.Random(11).randrange(mod)
    sys_ = _check_r1cs(curve, 2, 1, 3 + nbits, cons, hints, [[v, v] for v in (0, 1, mod - 1, rnd)])
    W = _solve_r1cs(sys_, [rnd, rnd], len(cons))[0]
    assert W[3:] == [(rnd >> i) & 1 for i in range(nbits)]
    with pytest.raises(solver.UnsatisfiedConstraintError) as e:  # a wrong public claim
        sys_.solve([rnd ^ 1, rnd])
    assert e.value.cid == nbits  # the recomposition constraint
    sys_.close()


# ------------------------------------------------- block and wave boundaries
@pytest.mark.parametrize("curve", CURVES)
def test_300_single_output_hints_in_a_hint_only_level(curve):
    """More than one 256-thread block of the evaluate kernel; level 0 holds only
    hints, level 1 the constraint that reads them all."""
    mod = _mod(curve)
    nin, n = 5, 300  # ONE + 4 secrets
    kinds = (hr.INV_ZERO, hr.ITH_BIT, hr.MIN_OUTPUT, hr.IS_LESS_OUTPUT)
    hints = []
    for i in range(n):
        k = kinds[i % 4]
        ins = [[(1 + i % 4, 1 + i)]]
        if k == hr.ITH_BIT:
            ins.append([(0, i % 256)])
        elif k != hr.INV_ZERO:
            ins.append([(1 + (i + 1) % 4, 3)])
        hints.append(hr.H(k, ins, nin + i, nin + i + 1, 0))
    s = nin + n
    cons = [([(nin + i, 1 + i) for i in range(n)], [(0, 1)], [(s, 1)])]
    lv = hr.levels_with_hints(nin, hr.r1cs_wires(cons), hints)
    assert lv == ([[], [0]], [list(range(n)), []])
    rng = random.Random(21)
    sys_ = _check_r1cs(curve, 1, 4, s + 1, cons, hints, [[rng.randrange(mod) for _ in range(4)]])
    assert sys_.schedule() == (False, 3, 0)  # evaluate + scatter, then the constraint level
    sys_.close()


@pytest.mark.parametrize("curve", CURVES)
def test_70_nbits_hints_of_65_outputs_beside_constraints(curve):
    """4,550 output threads whose hint boundaries straddle the 64-lane waves, in
    a level that also holds constraints."""
    mod = _mod(curve)
    nin, n, nout = 4, 70, 65
    base = nin + 2  # two level-0 constraints produce wires 4 and 5
    cons = [([(1, 1)], [(2, 1)], [(4, 1)]), ([(2, 5)], [(3, 1)], [(5, 7)])]
    hints = [hr.H(hr.N_BITS, [[(1 + i % 3, 1 + i), (0, i)]], base + i * nout, base + (i + 1) * nout, 2)
             for i in range(n)]
    nw = base + n * nout
    # level 1: a recomposition of the first hint's low 65 bits, shifted by a constraint wire
    cons.append(([(base + j, 1 << j) for j in range(nout)], [(4, 1)], [(nw, 1)]))
    lv = hr.levels_with_hints(nin, hr.r1cs_wires(cons), hints)
    assert lv == ([[0, 1], [2]], [list(range(n)), []])
    rng = random.Random(22)
    sys_ = _check_r1cs(curve, 2, 2, nw + 1, cons, hints, [[rng.randrange(mod) for _ in range(3)]])
    sys_.close()


# --------------------------------------------------------- input expressions
@pytest.mark.parametrize("curve", CURVES)
def test_input_expressions(curve):
    mod = _mod(curve)
    # wires: 0 ONE, 1 p (public), 2 s, 3 t (secret); internal from 4
    cons = [([(1, 1)], [(2, 1)], [(4, 1)])]                                # w4 = p s
    hints = [
        hr.H(hr.INV_ZERO, [[]], 5, 6, 1),                                   # an empty expression: 0
        hr.H(hr.N_BITS, [[]], 6, 9, 1),
        hr.H(hr.N_BITS, [[(0, 0b1011)]], 9, 14, 1),                         # a constant via wire 0
        hr.H(hr.N_TRITS, [[(hr.CONST_WIRE, 3 ** 5 + 2)]], 14, 21, 1),       # a constant term proper
        hr.H(hr.INV_ZERO, [[(3, 1)]], 21, 22, 1),                           # a coefficient of one
        hr.H(hr.MIN_OUTPUT, [[(2, 1), (3, 1)], [(4, 1)]], 22, 23, 1),
    ]
    # five terms: witness wires, an internal wire, an earlier hint's output, a constant
    hints.append(hr.H(hr.N_NAF, [[(1, 3), (3, mod - 2), (4, 1), (21, 12345), (0, 77)]], 23, 23 + 258, 1))
    nw = 23 + 258
    rng = random.Random(31)
    wits = [[rng.randrange(mod) for _ in range(3)] for _ in range(2)] + [[0, 0, 0]]
    sys_ = _check_r1cs(curve, 2, 2, nw, cons, hints, wits)
    W = _solve_r1cs(sys_, wits[0], 1)[0]
    assert W[5:9] == [0, 0, 0, 0] and W[9:14] == [1, 1, 0, 1, 0] and W[14:21] == [2, 0, 0, 0, 0, 1, 0]
    sys_.close()


# ----------------------------------------------------- random mixed circuits
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("seed,zero", [(1, False), (2, False), (3, True), (4, True)])
def test_random_r1cs_with_hints(curve, seed, zero):
    mod = _mod(curve)
    rng = random.Random(1000 + seed)
    nbp, nbs = 3, 4
    cons, hints, nw = hr.random_circuit(rng, mod, nbp, nbs, 300, zero_divisor=zero)
    assert {h.hint_id for h in hints} == set(hr.KINDS)
    wit = [rng.randrange(mod) for _ in range(nbp - 1 + nbs)]
    _check_r1cs(curve, nbp, nbs, nw, cons, hints, [wit]).close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_scs_with_hints(curve, seed):
    from gnark_amd import solver
    mod = _mod(curve)
    rng = random.Random(2000 + seed)
    nbp, nbs = 3, 4
    cons, hints, nw = hr.random_scs_circuit(rng, mod, nbp, nbs, 300)
    assert {h.hint_id for h in hints} == set(hr.KINDS)
    wit = [rng.randrange(mod) for _ in range(nbp + nbs)]
    lv = hr.levels_with_hints(nbp + nbs, hr.scs_wires(cons), hints)
    W = hr.solve_scs_with_hints(mod, nw, cons, hints, wit, lv)
    sys_ = solver.SparseR1CS.from_constraints(nbp, nbs, nw, cons, curve=curve, hints=_hints(hints))
    got = [_vals(x.to_host(), curve) for x in sys_.solve(wit)]
    assert got[0] == W
    assert tuple(got[1:]) == tuple(sc.lro(W, cons, nbp))
    assert sys_.schedule()[0] is False
    sys_.close()


# -------------------------------------------------------------------- errors
def _two_hint_chain(mod):
    # wires: 0 ONE, 1 a; 2 = InvZero(a), 3 = InvZero(w2), 4 = w3 * 1
    cons = [([(3, 1)], [(0, 1)], [(4, 1)])]
    hints = [hr.H(hr.INV_ZERO, [[(1, 1)]], 2, 3, 0), hr.H(hr.INV_ZERO, [[(2, 1)]], 3, 4, 0)]
    return cons, hints


def test_hint_placed_too_late_is_reported():
    from gnark_amd import solver, GnarkAmdError
    cons, hints = _two_hint_chain(o.R)
    assert hr.levels_with_hints(2, hr.r1cs_wires(cons), hints) == ([[], [], [0]], [[0], [1], []])
    # hint 0 in the level of its consumer, hint 1: that one reads an unsolved wire
    sys_ = solver.R1CS.from_terms(1, 1, 5, cons, hints=_hints(hints), levels=[[], [], [0]],
                                  hint_levels=[[], [0, 1], []])
    with pytest.raises(GnarkAmdError) as e:
        sys_.solve([5])
    assert e.value.code == GG_ERR_INVALID_ARG
    assert "hint #1: input wire unsolved at its level (the levels do not match the system)" in str(e.value)
    sys_.close()
    # the right levels solve
    sys_ = solver.R1CS.from_terms(1, 1, 5, cons, hints=_hints(hints))
    assert _solve_r1cs(sys_, [5], 1)[0] == [1, 5, pow(5, -1, o.R), 5, 5]
    sys_.close()


def test_set_hints_argument_errors():
    from gnark_amd import solver, GnarkAmdError
    cons, hints = _two_hint_chain(o.R)

    def refuse(hs, code, text, **kw):
        with pytest.raises(GnarkAmdError) as e:
            solver.R1CS.from_terms(1, 1, 6, cons, hints=_hints(hs), **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    refuse([hints[0], hints[1]._replace(hint_id=hr.N_BITS, out_start=2, out_end=4)], GG_ERR_INVALID_ARG, "overlap")
    refuse([hints[0], hints[1]._replace(out_start=3, out_end=5)], GG_ERR_INVALID_ARG, "output(s)")  # arity
    refuse([hints[0], hints[1]._replace(hint_id=hr.N_BITS, out_start=1, out_end=4)], GG_ERR_INVALID_ARG,
           "input wire")                                           # an output range inside the inputs
    refuse([hints[0], hints[1]._replace(hint_id=hr.N_BITS, out_start=3, out_end=7)], GG_ERR_INVALID_ARG,
           "passes the wires")
    refuse([hints[0], hints[1]._replace(hint_id=0x12345678)], GG_ERR_UNSUPPORTED, "0x12345678")
    refuse([hints[0], hints[1]._replace(inputs=[[(2, 1)], [(1, 1)]])], GG_ERR_INVALID_ARG, "input(s)")  # arity
    refuse([hints[0], hints[1]._replace(inputs=[[(6, 1)]])], GG_ERR_INVALID_ARG, "wire id out of range",
           levels=[[], [], [0]], hint_levels=[[0], [1], []])
    refuse(hints, GG_ERR_INVALID_ARG, "every hint once", levels=[[], [], [0]], hint_levels=[[0], [0], []])
    refuse(hints, GG_ERR_INVALID_ARG, "levels", levels=[[], [], [0]], hint_levels=[[0], [1]])
    # twice, and after a solve
    sys_ = solver.R1CS.from_terms(1, 1, 5, cons, hints=_hints(hints))
    with pytest.raises(GnarkAmdError) as e:
        sys_.set_hints(sys_.hints, sys_.hint_levels, lambda k: 0)
    assert e.value.code == GG_ERR_INVALID_ARG and "already set" in str(e.value)
    sys_.close()
    rcs = o.cubic_r1cs()
    sys_ = solver.R1CS.from_terms(rcs.nb_public, rcs.nb_secret, rcs.nb_wires, rcs.constraints)
    sys_.solve([35, 3])
    assert sys_.schedule()[0] is True  # a hint-free handle keeps the strand schedule
    with pytest.raises(GnarkAmdError) as e:
        sys_.set_hints([], [[] for _ in sys_.levels], lambda k: 0)
    assert e.value.code == GG_ERR_INVALID_ARG and "already solved" in str(e.value)
    sys_.close()
    # the sparse-R1CS entry point runs the same checks
    with pytest.raises(GnarkAmdError) as e:
        solver.SparseR1CS.from_constraints(1, 1, 4, [(0, 1, 3, 1, 1, o.R - 1, 0, 0)], curve="bn254",
                                           hints=_hints([hr.H(0x12345678, [[(0, 1)]], 2, 3, 0)]))
    assert e.value.code == GG_ERR_UNSUPPORTED


# ---------------------------------------------------------------- end to end
def test_groth16_proof_from_a_solution_with_hints():
    """x != 0 and x < 2^8 (IsZero plus an 8-bit ToBinary) with the public
    y = x^2: the GPU solves with hints, the prover reads the resident solution,
    and the proof equals the oracle's on hint_ref's wires byte for byte."""
    from gnark_amd import backend, groth16, solver
    mod = o.R
    # wires: 0 ONE, 1 y (public), 2 x (secret), 3 m, 4 inv, 5..12 bits
    cons = [([(2, mod - 1)], [(4, 1)], [(3, 1), (0, mod - 1)]),   # (-x) inv = m - 1
            ([(2, 1)], [(3, 1)], [(0, 0)]),                       # x m = 0
            ([(3, 1)], [(0, 1)], [(0, 0)])]                       # m = 0: x != 0
    cons += [([(5 + i, 1)], [(0, 1), (5 + i, mod - 1)], [(0, 0)]) for i in range(8)]
    cons.append(([(5 + i, 1 << i) for i in range(8)], [(0, 1)], [(2, 1)]))  # x < 2^8
    cons.append(([(2, 1)], [(2, 1)], [(1, 1)]))                             # x x = y
    hints = [hr.H(hr.INV_ZERO, [[(2, 1)]], 4, 5, 0), hr.H(hr.N_BITS, [[(2, 1)]], 5, 13, 3)]
    rcs = o.R1CS(2, 1, 10, cons)
    assert rcs.nb_wires == 13
    x = 201
    lv = hr.levels_with_hints(3, hr.r1cs_wires(cons), hints)
    W, A, B, C = hr.solve_with_hints(mod, 13, cons, hints, [x * x, x], lv)
    tw = o.ToxicWaste(271828, 314159, 161803, 141421, 173205)
    pko, vk = o.setup(rcs, tw)
    assert pko.domain.log_n == 4
    r, s = 97531, 24680
    want = o.prove(rcs, pko, W, r, s)
    cat = lambda f, pts: b"".join(f(p) for p in pts)
    pk = groth16.ProvingKey(groth16.ProvingKeyData(
        log_n=pko.domain.log_n, g1_A=cat(o.g1_to_bytes, pko.g1_A), g1_B=cat(o.g1_to_bytes, pko.g1_B),
        g1_Z=cat(o.g1_to_bytes, pko.g1_Z), g1_K=cat(o.g1_to_bytes, pko.g1_K),
        alpha1=o.g1_to_bytes(pko.g1_alpha), beta1=o.g1_to_bytes(pko.g1_beta), delta1=o.g1_to_bytes(pko.g1_delta),
        g2_B=cat(o.g2_to_bytes, pko.g2_B), beta2=o.g2_to_bytes(pko.g2_beta), delta2=o.g2_to_bytes(pko.g2_delta),
        infinity_A=bytes(int(v) for v in pko.infinity_A), infinity_B=bytes(int(v) for v in pko.infinity_B),
        nb_public=rcs.nb_public))
    sys_ = solver.R1CS.from_terms(2, 1, 13, cons, hints=_hints(hints))
    sol = sys_.solve([x * x, x])
    assert _vals(sol.W.to_host(), "bn254") == W
    pr = groth16.prove(pk, sol, backend.with_amd_acceleration(), r=o.fr_to_bytes(r), s=o.fr_to_bytes(s))
    assert (pr.Ar, pr.Bs, pr.Krs) == (o.g1_to_bytes(want.Ar), o.g2_to_bytes(want.Bs), o.g1_to_bytes(want.Krs))
    proof = o.Proof(o.g1_from_bytes(pr.Ar), o.g2_from_bytes(pr.Bs), o.g1_from_bytes(pr.Krs))
    assert o.verify(proof, vk, [x * x])
    assert not o.verify(proof, vk, [x * x + 1])
    # x = 0 and x >= 2^8 do not solve
    with pytest.raises(solver.UnsatisfiedConstraintError) as e:
        sys_.solve([0, 0])
    assert e.value.cid == 2
    with pytest.raises(solver.UnsatisfiedConstraintError) as e:
        sys_.solve([256 * 256, 256])
    assert e.value.cid == 11
    sys_.close()
    pk.close()

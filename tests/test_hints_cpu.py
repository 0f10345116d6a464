"""gnark's built-in hints, the parts that need no GPU: the HintID table, the
library's host evaluation (gg_hint_eval_host: the code the kernels run) against
the from-spec restatement tests/hint_ref.py on both scalar fields, and the
mirror's hint-aware level builders.  Every comparison is exact."""
import random

import pytest

import hint_ref as hr

BN_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BLS_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FIELDS = [("bn254", BN_R), ("bls12-381", BLS_R)]
GG_ERR_INVALID_ARG, GG_ERR_UNSUPPORTED = 1, 4


def _values(mod, seed):
    rng = random.Random(seed)
    edge = [0, 1, 2, 3, mod - 1, (mod - 1) // 2, (mod - 1) // 2 + 1, 1 << 253]
    return edge, edge + [rng.randrange(mod) for _ in range(50)]


def test_hint_id_table():
    from gnark_amd import solver
    assert solver.HINT_IDS == {name: hid for hid, name in hr.GO_NAMES.items()}
    for hid, name in hr.GO_NAMES.items():
        assert solver.hint_id(name) == hid
        assert solver.hint_supported(hid) == (True, name)
    assert solver.hint_supported(0x12345678) == (False, None)
    # the BSB22 commitment hint is not one of them (those systems keep gnark's solver)
    assert not solver.hint_supported(solver.hint_id("github.com/consensys/gnark/constraint/bn254.bsb22CommitmentComputePlaceholder"))[0]


@pytest.mark.parametrize("curve,mod", FIELDS, ids=[c for c, _ in FIELDS])
def test_host_eval_inv_zero(curve, mod):
    from gnark_amd import solver
    for v in _values(mod, 1)[1]:
        assert solver.hint_eval_host(curve, hr.INV_ZERO, [v], 1) == hr.eval_hint(mod, hr.INV_ZERO, [v], 1)


@pytest.mark.parametrize("curve,mod", FIELDS, ids=[c for c, _ in FIELDS])
@pytest.mark.parametrize("kind,counts", [(hr.N_BITS, (1, 64, 254, 256, 300)), (hr.N_TRITS, (1, 40, 161, 170)),
                                         (hr.N_NAF, (1, 255, 256, 260))],
                         ids=["nBits", "nTrits", "nNaf"])
def test_host_eval_digits(curve, mod, kind, counts):
    from gnark_amd import solver
    for v in _values(mod, 2)[1]:
        for n in counts:
            assert solver.hint_eval_host(curve, kind, [v], n) == hr.eval_hint(mod, kind, [v], n), (hex(v), n)
    assert solver.hint_eval_host(curve, kind, [5], 0) == []


@pytest.mark.parametrize("curve,mod", FIELDS, ids=[c for c, _ in FIELDS])
def test_host_eval_ith_bit(curve, mod):
    from gnark_amd import solver
    for v in _values(mod, 3)[1]:
        for i in (0, 1, 253, 255, 256, 1 << 32, 1 << 64):
            assert solver.hint_eval_host(curve, hr.ITH_BIT, [v, i], 1) == hr.eval_hint(mod, hr.ITH_BIT, [v, i], 1)
    # [2^63, 2^64): 0 by definition (the reference panics there)
    assert solver.hint_eval_host(curve, hr.ITH_BIT, [mod - 1, 1 << 63], 1) == [0]
    assert solver.hint_eval_host(curve, hr.ITH_BIT, [mod - 1, (1 << 64) - 1], 1) == [0]


@pytest.mark.parametrize("curve,mod", FIELDS, ids=[c for c, _ in FIELDS])
def test_host_eval_comparisons(curve, mod):
    from gnark_amd import solver
    edge, vals = _values(mod, 4)
    pairs = [(a, b) for a in edge for b in edge] + list(zip(vals[8:], reversed(vals[8:])))
    for kind in (hr.MIN_OUTPUT, hr.IS_LESS_OUTPUT):
        for a, b in pairs:
            assert solver.hint_eval_host(curve, kind, [a, b], 1) == hr.eval_hint(mod, kind, [a, b], 1), (a, b)


def test_host_eval_errors():
    from gnark_amd import solver, GnarkAmdError
    for kind, (n_in, n_out) in hr.ARITY.items():
        with pytest.raises(GnarkAmdError) as e:
            solver.hint_eval_host("bn254", kind, [1] * (3 - n_in), 1)
        assert e.value.code == GG_ERR_INVALID_ARG
        if n_out is not None:
            with pytest.raises(GnarkAmdError) as e:
                solver.hint_eval_host("bn254", kind, [1] * n_in, 2)
            assert e.value.code == GG_ERR_INVALID_ARG
    with pytest.raises(GnarkAmdError) as e:
        solver.hint_eval_host("bls12-381", 0xDEADBEEF, [1], 1)
    assert e.value.code == GG_ERR_UNSUPPORTED and "0xdeadbeef" in str(e.value)


def _csr(cons):
    off, wires = [0], []
    for side3 in cons:
        for side in side3:
            wires += [w for w, _ in side]
            off.append(len(wires))
    return off, wires


def _same_levels(got, want):
    return [[sorted(x) for x in part] for part in got] == [[sorted(x) for x in part] for part in want]


@pytest.mark.parametrize("seed", range(6))
def test_mirror_hint_levels_match_ref(seed):
    from gnark_amd import solver
    rng = random.Random(100 + seed)
    cons, hints, nw = hr.random_circuit(rng, BN_R, 2, 3, 120)
    off, wires = _csr(cons)
    got = solver.compute_levels_with_hints(5, nw, off, wires, hints)
    want = hr.levels_with_hints(5, hr.r1cs_wires(cons), hints)
    assert len(got[0]) == len(got[1]) and _same_levels(got, want)
    assert sorted(i for lv in got[1] for i in lv) == list(range(len(hints)))
    scs, shints, snw = hr.random_scs_circuit(rng, BLS_R, 2, 3, 120)
    got = solver.compute_scs_levels_with_hints(5, snw, [w for k in scs for w in k[:3]], shints)
    assert _same_levels(got, hr.levels_with_hints(5, hr.scs_wires(scs), shints))


def test_hint_levels_place_outputs_above_the_deepest_input():
    """A hint on an internal wire sits one level above it, its consumer one
    above the hint; a hint on witness wires alone sits in level 0, before or
    after any constraint in instruction order."""
    from gnark_amd import solver
    # wires: 0 ONE, 1 a (witness), 2 = a*a, 3 = InvZero(w2), 4 = w3*a, 5 = InvZero(a)
    cons = [([(1, 1)], [(1, 1)], [(2, 1)]), ([(3, 1)], [(1, 1)], [(4, 1)])]
    hints = [hr.H(hr.INV_ZERO, [[(2, 1)]], 3, 4, 1), hr.H(hr.INV_ZERO, [[(1, 1)]], 5, 6, 2)]
    off, wires = _csr(cons)
    assert solver.compute_levels_with_hints(2, 6, off, wires, hints) == ([[0], [], [1]], [[1], [0], []])
    assert hr.levels_with_hints(2, hr.r1cs_wires(cons), hints) == ([[0], [], [1]], [[1], [0], []])


def test_hint_free_levels_unchanged():
    """compute_levels on a hint-free system: the values the suite pinned before
    hints existed, and the hint-aware builder with no hints agrees."""
    import r1cs_solver as rs
    from gnark_amd import solver
    rng = random.Random(5)
    cons = rs.random_circuit(rng, 2, 3, 60)
    off, wires = _csr(cons)
    got = solver.compute_levels(5, 65, off, wires)
    assert [sorted(x) for x in got] == [sorted(x) for x in rs.levels_of(5, cons)]
    cl, hl = solver.compute_levels_with_hints(5, 65, off, wires, [])
    assert cl == got and all(not x for x in hl)


def test_header_documents_the_hint_table():
    """include/gnark_amd.h lists every id with its Go name's tail."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gnark_amd.h")).read()
    for hid, name in hr.GO_NAMES.items():
        assert "0x%08x" % hid in src and name.rsplit("/", 1)[1] in src

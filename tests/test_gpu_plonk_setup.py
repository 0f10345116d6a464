"""PlonK Setup on the GPU (csrc/ecntt.hip, csrc/plonk_setup.hip): the EC-NTT
against the SRS trapdoor and against the oracle's field iDFT on degenerate
inputs, gg_plonk_setup against the restated setup.go (plonk_setup_ref.py), and
setup -> solve -> prove end to end against the two oracles.  Every comparison
is bytes-equal: affine coordinates and field elements are unique."""
import functools
import random

import numpy as np
import pytest

import plonk_prover_oracle as po
import plonk_setup_ref as ref
import scs_solver as ss
from plonk_circuits import FIELDS, m2b, srs

pytestmark = pytest.mark.gpu

CURVES = ("bls12-381", "bn254")
TAU = 0x5eed0123456789abcdef


@functools.lru_cache(maxsize=None)
def _srs(curve, log_n):
    """(pk.Kzg.G1[:n+3], the trapdoor [L_i(tau)]G), computed once per size"""
    return srs(log_n, TAU, curve)


def _group(curve):
    from gnark_amd import msm
    return msm.BLS12_381_G1 if curve == "bls12-381" else msm.G1


def _mont(F, xs):
    return b"".join(m2b(x % F.R * F.MONT % F.R) for x in xs)


def _points(curve, scalars):
    """[s_j]G by the fixed-base comb (gg_batch_scalar_mul)"""
    from gnark_amd import msm
    F = FIELDS[curve]
    return msm.batch_scalar_mul(_group(curve), F.g1_to_bytes(F.cv.G1), _mont(F, scalars), len(scalars))


# ------------------------------------------------------------ EC-NTT
@pytest.mark.parametrize("curve,log_n", [(c, k) for c in CURVES for k in (1, 2, 5, 10)] +
                         [("bls12-381", 13), ("bn254", 15)])
def test_ecntt_against_the_trapdoor(curve, log_n):
    """1, 2, 5, 10: one block, several blocks, every thread order of a stage
    (block-major, butterfly-major for short blocks); 13: butterfly-major stages
    with long blocks (stage 6 on); 15: above 2^14 points a thread of the
    normalisation owns more than one point."""
    from gnark_amd import kzg
    pt = FIELDS[curve].pt
    canon, lag = _srs(curve, log_n)
    got = kzg.to_lagrange_g1(canon[:pt << log_n], log_n, curve=curve)
    assert got == lag


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("mode,chunk", [("naf", None), ("window", None), ("window", 200), ("window", 128)])
def test_ecntt_multiplication_variants_agree(curve, mode, chunk, monkeypatch):
    """The two twiddle products -- non-adjacent form, and signed 4-bit windows
    with their per-thread table (the default) -- GG_ECNTT_MUL -- and the window
    stages cut into several launches that share one table (chunks of 256 and
    of 128 threads for the 512 butterflies of 2^10)."""
    from gnark_amd import kzg
    monkeypatch.setenv("GG_ECNTT_MUL", mode)
    if chunk:
        monkeypatch.setenv("GG_ECNTT_WINDOW_CHUNK", str(chunk))
    pt = FIELDS[curve].pt
    for log_n in (3, 10):
        canon, lag = _srs(curve, log_n)
        assert kzg.to_lagrange_g1(canon[:pt << log_n], log_n, curve=curve) == lag


def _degenerate(kind, n, F, rng):
    R = F.R
    w = F.cv.omega(n)
    if kind == "all_equal":      # one point and n - 1 infinities; every butterfly has a = b
        return [12345] * n
    if kind == "unit":           # the inputs are mostly infinity
        return [0] * 5 + [777] + [0] * (n - 6)
    if kind == "tau_in_domain":  # tau = w^3: L_i(tau) = [i == 3]
        return [pow(w, 3 * j, R) for j in range(n)]
    if kind == "pairs":          # (s, -s): a + b = infinity in the first stage
        h = [rng.randrange(R) for _ in range(n // 2)]
        return h + [(R - x) % R for x in h]
    s = [rng.randrange(R) for _ in range(n)]  # random scalars with zeros
    for j in range(0, n, 3):
        s[j] = 0
    return s


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [4, 10])
@pytest.mark.parametrize("kind", ["all_equal", "unit", "tau_in_domain", "pairs", "zeros"])
def test_ecntt_degenerate_inputs(curve, log_n, kind):
    from gnark_amd import kzg
    F = FIELDS[curve]
    n = 1 << log_n
    s = _degenerate(kind, n, F, random.Random(log_n * 31 + len(kind)))
    want_scalars = po.interpolate(s, F.cv.omega(n), F.R)  # iDFT(s)_i = (1/n) sum_j s_j w^(-ij)
    if kind == "all_equal":
        assert want_scalars == [12345] + [0] * (n - 1)
    if kind == "tau_in_domain":
        assert want_scalars == [int(i == 3) for i in range(n)]
    got = kzg.to_lagrange_g1(_points(curve, s), log_n, curve=curve)
    assert got == _points(curve, want_scalars)


@pytest.mark.parametrize("curve", CURVES)
def test_ecntt_device_buffers_and_aliasing(curve):
    from gnark_amd import kzg
    from gnark_amd._lib import DeviceBuffer
    log_n, pt = 5, FIELDS[curve].pt
    canon, lag = _srs(curve, log_n)
    src = DeviceBuffer.from_host(canon[:pt << log_n])
    out = kzg.to_lagrange_g1(src, log_n, curve=curve, out_device=True)
    assert out.to_host() == lag
    assert src.to_host() == canon[:pt << log_n]        # the input is left alone
    assert kzg.to_lagrange_g1(src, log_n, curve=curve) == lag  # device in, host out
    same = kzg.to_lagrange_g1(src, log_n, curve=curve, out=src)  # in == out
    assert same is src and src.to_host() == lag


# ------------------------------------------------------------ Setup against the reference
def _setup_case(curve, size_system, nbp, n_cmt, seed):
    """A random sparse R1CS in which wire 0 is reused heavily and some wires
    are unused (Setup does not need it satisfiable), with its commitments."""
    F = FIELDS[curve]
    rng = random.Random(seed)
    n_cons = size_system - nbp
    cons, _flags, nw = ss.random_circuit(rng, F.R, nbp, 3, n_cons)
    cons = ss.fill_assertions(F.R, cons, [rng.randrange(F.R) for _ in range(nbp + 3)])
    out = []
    for k in cons:
        k = list(k)
        if rng.random() < 0.35:
            k[rng.randrange(3)] = 0
        out.append(tuple(k))
    nw += 5  # wires no constraint names
    cmts = []
    for _ in range(n_cmt):
        committed = sorted(rng.sample(range(n_cons), min(n_cons, rng.randrange(1, 6))))
        cmts.append((committed, rng.randrange(n_cons)))
    return out, nw, cmts


def _reference(curve, cons, nbp, nw, cmts):
    """every read part (bytes) and the Lagrange-regular trace (ints) by plonk_setup_ref"""
    F = FIELDS[curve]
    R = F.R
    n, big = ref.init_domains(len(cons), nbp)
    w, u = F.cv.omega(n), F.cv.fr_gen
    ql, qr, qm, qo, qk, qcp = ref.build_trace(R, cons, nbp, cmts)
    perm = ref.build_permutation(cons, nbp, nw)
    s1, s2, s3 = ref.permutation_polynomials(R, perm, n, w, u)
    lag = dict(ql=ql, qr=qr, qm=qm, qo=qo, qk=qk, s1=s1, s2=s2, s3=s3)
    canon = {k: po.interpolate(v, w, R) for k, v in lag.items()}
    qcp_c = [po.interpolate(v, w, R) for v in qcp]
    parts = {k: _mont(F, v) for k, v in canon.items()}
    for j, v in enumerate(qcp_c):
        parts[("qcp", j)] = _mont(F, v)
    parts["perm"] = np.array(perm, np.int64).tobytes()
    return n, big, lag, qcp, perm, canon, qcp_c, parts


def _system(curve, cons, nbp, nw):
    """the raw arrays of gg_scs_create without a solver handle"""
    from gnark_amd import fr
    F = FIELDS[curve]
    mont = fr.bls_fr_mont if curve == "bls12-381" else fr.fr_mont
    table, index, wires, qidx = [], {}, [], []
    for xa, xb, xc, *qs in cons:
        wires += [xa, xb, xc]
        for k in qs:
            k %= F.R
            if k not in index:
                index[k] = len(table)
                table.append(k)
            qidx.append(index[k])
    return (nw, nbp, np.array(wires, np.uint32), np.array(qidx, np.uint32), b"".join(mont(k) for k in table))


@pytest.mark.parametrize("curve,size_system,nbp,n_cmt", [
    ("bls12-381", 2, 0, 0), ("bn254", 2, 0, 0),
    ("bls12-381", 5, 3, 1), ("bn254", 5, 3, 1),
    ("bls12-381", 6, 3, 0),
    ("bls12-381", 64, 0, 2), ("bn254", 64, 0, 2),
    ("bn254", 65, 3, 1),
    ("bls12-381", 3000, 3, 2),
])
def test_setup_matches_the_reference(curve, size_system, nbp, n_cmt):
    from gnark_amd import plonk_prover as pp
    F = FIELDS[curve]
    cons, nw, cmts = _setup_case(curve, size_system, nbp, n_cmt, 900 + size_system)
    n, big, _lag, _qcp, _perm, canon, qcp_c, parts = _reference(curve, cons, nbp, nw, cmts)
    log_n = n.bit_length() - 1
    kzg_g1, kzg_lag = _srs(curve, log_n)
    pk, vk, sd = pp.setup(_system(curve, cons, nbp, nw), kzg_g1, commitments=cmts, curve=curve, keep=True)
    assert (sd.log_n, sd.log_big, sd.n_cmt, sd.lagrange_computed) == (log_n, big.bit_length() - 1, n_cmt, True)
    assert (pk.log_n, pk.big_log) == (sd.log_n, sd.log_big)
    for part, want in parts.items():
        assert sd.read(part) == want, part
    assert sd.read("lagrange") == kzg_lag
    t = sd.timings()
    assert t["total"] > 0 and t["ecntt_stages"] > 0
    # the vk digests: the key's own commitTrace against [p(tau)]G
    cv, g = F.cv, F.g1_from_bytes

    def com(c):
        return cv.mul(cv.G1, po.horner(c, TAU, cv.R))
    assert [g(x) for x in vk.S] == [com(canon[k]) for k in ("s1", "s2", "s3")]
    assert [g(x) for x in (vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk)] == [com(canon[k]) for k in ("ql", "qr", "qm", "qo", "qk")]
    assert [g(x) for x in vk.Qcp] == [com(c) for c in qcp_c]
    assert (vk.size, vk.nb_public, vk.commitment_indexes) == (n, nbp, [c[1] for c in cmts])
    pk.close()
    sd.close()


@pytest.mark.parametrize("curve", CURVES)
def test_setup_with_the_callers_lagrange_srs(curve):
    """kzg_lagrange_g1 given: used as it is; None: the EC-NTT's equals the trapdoor's."""
    from gnark_amd import plonk_prover as pp
    cons, nw, cmts = _setup_case(curve, 20, 2, 0, 77)
    kzg_g1, kzg_lag = _srs(curve, 5)
    marked = bytearray(kzg_lag)
    marked[:FIELDS[curve].pt] = bytes(FIELDS[curve].pt)  # recognisable: the first point replaced by infinity
    system = _system(curve, cons, 2, nw)
    given = pp.SetupData(*system, kzg_g1, bytes(marked), cmts, curve)
    assert not given.lagrange_computed and given.read("lagrange") == bytes(marked)
    assert given.timings()["ecntt_stages"] == 0
    computed = pp.SetupData(*system, kzg_g1, None, cmts, curve)
    assert computed.lagrange_computed and computed.read("lagrange") == kzg_lag
    for part in ("ql", "s3", "perm"):
        assert given.read(part) == computed.read(part)
    given.close()
    computed.close()


# ------------------------------------------------------------ end to end
def _ints(b, F):
    return [int.from_bytes(b[i:i + 32], "little") * F.MINV % F.R for i in range(0, len(b), 32)]


def _proof_dict(F, proof):
    g = F.g1_from_bytes
    return {"LRO": [g(x) for x in proof.LRO], "Z": g(proof.Z), "H": [g(x) for x in proof.H],
            "batched_H": g(proof.batched_H), "claimed": list(proof.claimed_values), "zs_H": g(proof.z_shifted_H),
            "zu": proof.z_shifted_value, "bsb22": [g(x) for x in proof.bsb22]}


@pytest.mark.parametrize("curve,nbp,n_cons", [("bls12-381", 2, 100), ("bn254", 3, 2)])
def test_setup_solve_prove_end_to_end(curve, nbp, n_cons):
    """setup(...) builds the key from the solver's own system, SparseR1CS.solve
    leaves L, R, O in HBM (wire-0 padding, evaluateLROSmallDomain), prove runs:
    the trapdoor verifier accepts and rejects a wrong public input, and the proof
    equals the oracle prover's on the key the oracle makes from the reference's
    trace and permutation.  BN254 runs sizeSystem = 5: n = 8 with the 8n domain."""
    from test_oracle_plonk_prover import blinding
    from gnark_amd import plonk_prover as pp, solver
    F = FIELDS[curve]
    cv = F.cv
    rng = random.Random(40 + n_cons)
    nbs = 3
    cons, flags, nw = ss.random_circuit(rng, F.R, nbp, nbs, n_cons)
    wit = [rng.randrange(F.R) for _ in range(nbp + nbs)]
    cons = ss.fill_assertions(F.R, cons, wit)
    n, big, lag, qcp, perm, _canon, _qcp_c, _parts = _reference(curve, cons, nbp, nw, [])
    log_n, log_big = n.bit_length() - 1, big.bit_length() - 1
    kzg_g1, _ = _srs(curve, log_n)
    sys_ = solver.SparseR1CS.from_constraints(nbp, nbs, nw, cons, curve=curve)
    pk, vk = pp.setup(sys_, kzg_g1)
    assert (pk.log_n, pk.big_log) == (log_n, log_big)
    _W, L, Rv, O = sys_.solve(wit)  # DeviceBuffers
    pub = wit[:nbp]
    got = pp.prove(pk, L, Rv, O, rng=random.Random(5), public=pub)
    key = po.setup(cv, log_n, lag["ql"], lag["qr"], lag["qm"], lag["qo"], lag["qk"], lag["s1"], lag["s2"],
                   lag["s3"], qcp, perm, nbp, [], TAU, big_log=log_big)
    g = F.g1_from_bytes
    assert [g(x) for x in vk.S] == key["vk"]["S"]
    assert [g(x) for x in (vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk)] == [key["vk"][k] for k in ("Ql", "Qr", "Qm", "Qo", "Qk")]
    pr = _proof_dict(F, got)
    assert po.verify_trapdoor(key, pr, pub)
    assert not po.verify_trapdoor(key, pr, [pub[0] + 1] + pub[1:])
    if curve == "bls12-381":
        import bls12_381_oracle as blo
        from plonk_circuits import to_oracle
        opr, ovk = to_oracle(pk, got)
        assert blo.plonk_verify_trapdoor(opr, ovk, TAU, public=pub)
        assert not blo.plonk_verify_trapdoor(opr, ovk, TAU, public=[pub[0] + 1] + pub[1:])
    nb = 32 * n
    want = po.prove(key, _ints(L.to_host(nb), F), _ints(Rv.to_host(nb), F), _ints(O.to_host(nb), F), pub, [],
                    blinding(5, F.R))
    assert pr == {k: want[k] for k in pr}
    if curve == "bls12-381":  # a multi-part key through gg_plonk_setup_pk: the same proof
        pkm, _ = pp.setup(sys_, kzg_g1, devices=[0, 0])
        assert len(pkm.devices()) == 2
        assert pp.prove(pkm, L, Rv, O, rng=random.Random(5), public=pub) == got
        pkm.close()
    pk.close()
    sys_.close()

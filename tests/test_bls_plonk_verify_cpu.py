"""PlonK Verify and the KZG opening check over BLS12-381 on the host path
(gg_plonk_verify_batch_bls12_381_host, gg_kzg_verify_bls12_381_host: the
per-proof functions the kernels run, in a loop on the CPU) against the Python
restatement of verify.go (bls_plonk_verify_ref.py) and the oracle's trapdoor
verifier, on proofs made by the oracle prover.  No GPU.

The reference costs about 2 s per accepted proof, so the corruptions are one
test each and share one host batch of the library."""
import ctypes
import hashlib
import random

import pytest

import bls12_381_oracle as o
import bls_plonk_verify_ref as ref
import plonk_prover_oracle as po
from bls_pairing_ref import g1_off_curve, g1_outside_subgroup, g2_off_twist, twist_point_outside_subgroup
from plonk_circuits import Circuit
from test_oracle_plonk_prover import blinding, oracle_key, oracle_solve

R = o.R
OK, MALFORMED, QUOTIENT, KZG = ref.OK, ref.MALFORMED, ref.QUOTIENT, ref.KZG
CASES = [(3, 0, 0), (4, 1, 0), (5, 2, 1), (5, 0, 2)]
G1 = o.g1_to_bytes(o.G1_GEN)
_made = {}


def instance(log_n, nb_public, n_cmt, hashes=(None, None)):
    """(oracle key, key dict, tau, proof, public inputs), made once per case"""
    k = (log_n, nb_public, n_cmt, hashes)
    if k not in _made:
        circ = Circuit(log_n, 60 + log_n, nb_public=nb_public, n_cmt=n_cmt, curve="bls12-381")
        tau = random.Random(log_n + 1).randrange(2, R)
        key = oracle_key(circ, tau)
        L, Rv, O, pub, cmts = oracle_solve(circ, key, 11)
        pr = po.prove(key, L, Rv, O, pub, cmts, blinding(6, R), challenge_hash=hashes[0], folding_hash=hashes[1])
        _made[k] = (key, ref.key_dict(key), tau, pr, list(pub))
    return _made[k]


def lib_key(kd, tau):
    from gnark_amd import plonk_verify as pv
    return pv.Bls12381VerifyingKey(ref.lib_vk(kd), G1, ref.g2_bytes(tau))


def small_order_point():
    """T = [r] g1_outside_subgroup(): on the curve, of cofactor order, not the infinity"""
    t = ref.g1_mul_unreduced(g1_outside_subgroup(), R)
    assert t is not o.INF and o.on_curve(t) and not ref.in_subgroup(t)
    return t


def corruptions(pr, pub):
    """(name, proof, public inputs, expected status) of the (5, 2, 1) proof: the
    BN254 list, then the two cases the cofactor adds"""
    def mod(**kw):
        q = dict(pr)
        q.update(kw)
        return q

    def claimed(j, v):
        c = list(pr["claimed"])
        c[j] = v
        return c
    G = o.G1_GEN
    return [
        ("claimed[2] + 1", mod(claimed=claimed(2, (pr["claimed"][2] + 1) % R)), pub, QUOTIENT),
        ("zu + 1", mod(zu=(pr["zu"] + 1) % R), pub, QUOTIENT),
        ("public input + 1", pr, [pub[0], (pub[1] + 1) % R], QUOTIENT),
        ("Z + G", mod(Z=o.g1_add(pr["Z"], G)), pub, QUOTIENT),
        ("claimed[7] + 1", mod(claimed=claimed(7, (pr["claimed"][7] + 1) % R)), pub, KZG),
        ("batched_H + G", mod(batched_H=o.g1_add(pr["batched_H"], G)), pub, KZG),
        ("zs_H + G", mod(zs_H=o.g1_add(pr["zs_H"], G)), pub, KZG),
        ("point off the curve", mod(LRO=[pr["LRO"][0], g1_off_curve(5), pr["LRO"][2]]), pub, MALFORMED),
        ("claimed value = r", mod(claimed=claimed(3, R)), pub, MALFORMED),
        ("point outside the subgroup", mod(H=[pr["H"][0], pr["H"][1], g1_outside_subgroup()]), pub, MALFORMED),
        ("zs_H + T, T of cofactor order", mod(zs_H=o.g1_add(pr["zs_H"], small_order_point())), pub, MALFORMED),
    ]


N_CORRUPTIONS = 11
I_QUOTIENT, I_KZG, I_OFF_CURVE, I_OUTSIDE, I_SMALL_ORDER = 0, 6, 7, 9, 10


def packed(pr):
    """the library's bytes of an oracle proof; a scalar >= r keeps its limbs"""
    from gnark_amd import plonk_prover as pp
    big = [j for j, v in enumerate(pr["claimed"]) if v >= R]
    q = dict(pr)
    q["claimed"] = [v % R for v in pr["claimed"]]
    b = bytearray(pp.proof_bytes(ref.lib_proof(q), "bls12-381"))
    nc = len(pr["bsb22"])
    for j in big:
        off = 96 * (8 + nc) + 32 * j
        b[off:off + 32] = pr["claimed"][j].to_bytes(32, "little")
    return bytes(b)


def corruption_batch():
    """(cases, the library's host verdicts of every case followed by the good proof), computed once"""
    if "corruption_batch" not in _made:
        from gnark_amd import plonk_verify as pv
        _, kd, tau, pr, pub = instance(5, 2, 1)
        cases = corruptions(pr, pub)
        assert len(cases) == N_CORRUPTIONS
        vk = lib_key(kd, tau)
        got = pv.verify_batch([packed(q) for _, q, _, _ in cases] + [packed(pr)], vk,
                              [w for _, _, w, _ in cases] + [pub], host=True)
        vk.close()
        _made["corruption_batch"] = (cases, got)
    return _made["corruption_batch"]


@pytest.mark.parametrize("log_n,nb_public,n_cmt", CASES)
def test_oracle_proofs_verify(log_n, nb_public, n_cmt):
    from gnark_amd import plonk_verify as pv
    key, kd, tau, pr, pub = instance(log_n, nb_public, n_cmt)
    vk = lib_key(kd, tau)
    assert vk.n_commitments == n_cmt and vk.curve == "bls12-381"
    assert pv.verify_batch([ref.lib_proof(pr)], vk, [pub], host=True) == [OK]
    pv.verify(ref.lib_proof(pr), vk, pub, host=True)
    assert ref.verify(kd, ref.g2_pair(tau), pr, pub) == OK
    assert po.verify_trapdoor(key, pr, pub)
    vk.close()


def test_corruption_batch_as_a_whole():
    cases, got = corruption_batch()
    assert got == [st for _, _, _, st in cases] + [OK]


@pytest.mark.parametrize("i", range(N_CORRUPTIONS))
def test_every_corruption(i):
    """the library's verdict is the reference's, which is the expected one"""
    key, kd, tau, _, _ = instance(5, 2, 1)
    cases, got = corruption_batch()
    name, q, w, st = cases[i]
    g2 = ref.g2_pair(tau)
    assert ref.verify(kd, g2, q, w) == st, name
    assert got[i] == st, name
    if st != MALFORMED:
        assert not po.verify_trapdoor(key, q, w), name
    if i == I_SMALL_ORDER:
        # only the subgroup test can catch it: the pairing kills T, everything else accepts the proof
        assert ref.verify(kd, g2, q, w, subgroup_check=False) == OK


def test_verify_raises_and_witness_checks():
    from gnark_amd import plonk_verify as pv
    _, kd, tau, pr, pub = instance(5, 2, 1)
    cases, _ = corruption_batch()
    vk = lib_key(kd, tau)
    with pytest.raises(pv.VerifyError, match="claimed quotient is not as expected") as e:
        pv.verify(packed(cases[I_QUOTIENT][1]), vk, pub, host=True)
    assert e.value.status == QUOTIENT
    with pytest.raises(pv.VerifyError, match="can't verify opening proof") as e:
        pv.verify(packed(cases[I_KZG][1]), vk, pub, host=True)
    assert e.value.status == KZG
    with pytest.raises(pv.VerifyError, match="invalid proof") as e:
        pv.verify(packed(cases[I_OUTSIDE][1]), vk, pub, host=True)
    assert e.value.status == MALFORMED
    # a witness element >= r, by its limbs
    wit = o.fr_to_bytes(pub[0]) + R.to_bytes(32, "little")
    assert pv.verify_batch([packed(pr)], vk, [wit], host=True) == [MALFORMED]
    # a coordinate >= p, by its limbs
    b = bytearray(packed(pr))
    b[0:48] = o.P.to_bytes(48, "little")
    assert pv.verify_batch([bytes(b)], vk, [pub], host=True) == [MALFORMED]
    with pytest.raises(ValueError, match="invalid witness size"):
        pv.verify(packed(pr), vk, pub + [1], host=True)
    with pytest.raises(ValueError, match="bytes, the key's proofs have"):
        pv.verify(packed(pr)[:-32], vk, pub, host=True)
    vk.close()


def test_large_batch_on_the_host_threads():
    """130 proofs: the transcripts run on several host threads; corruptions at the
    first, a middle and the last position"""
    from gnark_amd import plonk_verify as pv
    _, kd, tau, pr, pub = instance(5, 2, 1)
    vk = lib_key(kd, tau)
    cases = corruptions(pr, pub)
    good = packed(pr)
    proofs, wits, want = [good] * 130, [pub] * 130, [OK] * 130
    for pos, c in ((0, I_KZG), (64, I_QUOTIENT), (129, I_SMALL_ORDER)):
        proofs[pos], wits[pos], want[pos] = packed(cases[c][1]), cases[c][2], cases[c][3]
    assert pv.verify_batch(proofs, vk, wits, host=True) == want
    vk.close()


def test_hash_option():
    from gnark_amd import plonk_verify as pv
    h = hashlib.blake2s
    key, kd, tau, pr, pub = instance(4, 1, 0, (h, h))
    vk = lib_key(kd, tau)
    p = ref.lib_proof(pr)
    assert pv.verify_batch([p], vk, [pub], challenge_hash=h, folding_hash=h, host=True) == [OK]
    assert ref.verify(kd, ref.g2_pair(tau), pr, pub, h, h) == OK
    assert pv.verify_batch([p], vk, [pub], host=True) != [OK]
    assert pv.verify_batch([p], vk, [pub], challenge_hash=h, host=True) != [OK]
    assert pv.verify_batch([p], vk, [pub], folding_hash=h, host=True) != [OK]
    vk.close()


def kzg_cases(tau):
    """(digest, quotient, point, value, expected) over the SRS of tau: a degree-7
    polynomial, a wrong value, a constant (H at infinity), z = 0, y = 0"""
    rnd = random.Random(77)
    f = [rnd.randrange(R) for _ in range(8)]
    G = o.G1_GEN

    def commit(c):
        return o.g1_mul(G, po.horner(c, tau, R)) if po.horner(c, tau, R) else o.INF

    def open_(c, z):
        y = po.horner(c, z, R)
        q = po._div_x_minus_a(c, y, z, R)
        return commit(c), (commit(q) if q else o.INF), z, y
    z = rnd.randrange(R)
    good = open_(f, z)
    root = rnd.randrange(1, R)
    g = po._div_x_minus_a(f, po.horner(f, root, R), root, R)   # f = g (X - root) + f(root)
    vanishing = [(-c * root + d) % R for c, d in zip(g + [0], [0] + g)]  # g (X - root): y = 0 at root
    assert po.horner(vanishing, root, R) == 0
    return [good + (True,), (good[0], good[1], z, (good[3] + 1) % R, False), open_([5], z) + (True,),
            open_(f, 0) + (True,), open_(vanishing, root) + (True,)]


def kzg_edge_cases(tau):
    """a digest off the curve; a quotient outside the subgroup (H + T still satisfies the pairing equation)"""
    good = kzg_cases(tau)[0]
    return [(g1_off_curve(3), good[1], good[2], good[3], False),
            (good[0], o.g1_add(good[1], small_order_point()), good[2], good[3], False),
            (g1_outside_subgroup(), good[1], good[2], good[3], False)]


def test_kzg_verify_host():
    from gnark_amd import kzg
    tau = 0x1234567890abcdef1234567
    g2 = ref.g2_pair(tau)
    cases = kzg_cases(tau)
    assert cases[2][1] is o.INF and cases[3][2] == 0 and cases[4][3] == 0
    edge = kzg_edge_cases(tau)
    b = o.g1_to_bytes
    both = cases + edge
    got = kzg.verify(G1, ref.g2_bytes(tau), [b(c[0]) for c in both], [b(c[1]) for c in both],
                     [c[2] for c in both], [c[3] for c in both], host=True, curve="bls12-381")
    assert got == [c[4] for c in both]
    for c in both:
        assert ref.kzg_check(g2, c[0], c[1], c[2], c[3]) == c[4]
    # the quotient with a cofactor-order component is caught by the subgroup test alone
    assert ref.kzg_check(g2, *edge[1][:4], subgroup_check=False)
    with pytest.raises(ValueError, match="curve must be"):
        kzg.verify(G1, ref.g2_bytes(tau), [], [], [], [], host=True, curve="bw6-761")
    with pytest.raises(ValueError, match="96 bytes"):
        kzg.verify(G1[:64], ref.g2_bytes(tau), [b(cases[0][0])], [b(cases[0][1])], [1], [2], host=True,
                   curve="bls12-381")


def _create(**over):
    """gg_plonk_vk_create_bls12_381 on the (5, 2, 1) key with some arguments replaced -> (rc, message)"""
    from gnark_amd import _lib, fr
    _, kd, tau, _, _ = instance(5, 2, 1)
    b = o.g1_to_bytes
    a = dict(size=kd["n"], generator=fr.bls_fr_mont(kd["omega"]), coset_shift=fr.bls_fr_mont(kd["u"]),
             S=b"".join(b(s) for s in kd["S"]), Q=b"".join(b(kd[q]) for q in ("Ql", "Qr", "Qm", "Qo", "Qk")),
             Qcp=b"".join(b(q) for q in kd["Qcp"]), n_cmt=1, idx=(ctypes.c_uint32 * 1)(*kd["cmt_idx"]),
             nb_public=kd["nb_public"], kzg_g1=G1, kzg_g2=ref.g2_bytes(tau))
    a.update(over)
    h = ctypes.c_void_p()
    p = _lib.ptr
    rc = _lib.lib.gg_plonk_vk_create_bls12_381(a["size"], p(a["generator"]), p(a["coset_shift"]), p(a["S"]),
                                               p(a["Q"]), p(a["Qcp"]), a["n_cmt"], a["idx"], a["nb_public"],
                                               p(a["kzg_g1"]), p(a["kzg_g2"]), ctypes.byref(h))
    msg = _lib.lib.gg_last_error().decode() if rc else ""
    if rc == 0:
        _lib.lib.gg_plonk_vk_destroy_bls12_381(h)
    return rc, msg


def test_key_refusals():
    from gnark_amd import _lib, plonk_verify as pv
    _, kd, tau, _, _ = instance(5, 2, 1)
    assert _create() == (0, "")
    for name in ("generator", "coset_shift", "S", "Q", "Qcp", "idx", "kzg_g1", "kzg_g2"):
        rc, msg = _create(**{name: None})
        want = "commitment_indexes" if name == "idx" else name
        assert rc == 1 and f"null argument: {want}" in msg, (name, msg)
    assert _lib.lib.gg_plonk_vk_create_bls12_381(8, None, None, None, None, None, 0, None, 0, None, None, None) == 1
    assert "null argument: out" in _lib.lib.gg_last_error().decode()
    for size in (0, 1, 24):
        rc, msg = _create(size=size)
        assert rc == 1 and "power of two" in msg, msg
    rc, msg = _create(n_cmt=-1)
    assert rc == 1 and "n_cmt" in msg
    rc, msg = _create(idx=(ctypes.c_uint32 * 1)(kd["n"] - kd["nb_public"]))
    assert rc == 1 and "commitment index" in msg
    rc, msg = _create(generator=R.to_bytes(32, "little"))
    assert rc == 1 and "generator is zero or >= r" in msg
    off, out = o.g1_to_bytes(g1_off_curve(9)), o.g1_to_bytes(g1_outside_subgroup())
    good_s = b"".join(o.g1_to_bytes(s) for s in kd["S"])
    good_q = b"".join(o.g1_to_bytes(kd[q]) for q in ("Ql", "Qr", "Qm", "Qo", "Qk"))
    rc, msg = _create(S=good_s[:96] + off + good_s[192:])
    assert rc == 1 and "S[1] is not on the curve" in msg, msg
    rc, msg = _create(S=good_s[:192] + out)
    assert rc == 1 and "S[2] is not in the r-torsion" in msg, msg
    rc, msg = _create(Q=good_q[:96] + out + good_q[192:])
    assert rc == 1 and "Qr is not in the r-torsion" in msg, msg
    rc, msg = _create(Qcp=off)
    assert rc == 1 and "Qcp[0] is not on the curve" in msg, msg
    rc, msg = _create(Qcp=o.g1_to_bytes(small_order_point()))
    assert rc == 1 and "Qcp[0] is not in the r-torsion" in msg, msg
    rc, msg = _create(kzg_g1=off)
    assert rc == 1 and "kzg_g1 is not on the curve" in msg, msg
    rc, msg = _create(kzg_g1=out)
    assert rc == 1 and "kzg_g1 is not in the r-torsion" in msg, msg
    g2 = ref.g2_bytes(tau)
    rc, msg = _create(kzg_g2=g2[:192] + bytes(192))
    assert rc == 1 and "kzg_g2[1] is the point at infinity" in msg, msg
    rc, msg = _create(kzg_g2=o.g2_to_bytes(g2_off_twist(3)) + g2[192:])
    assert rc == 1 and "kzg_g2[0] is not on the twist" in msg, msg
    rc, msg = _create(kzg_g2=g2[:192] + o.g2_to_bytes(twist_point_outside_subgroup(3)))
    assert rc == 1 and "kzg_g2[1] is not in the r-torsion" in msg, msg
    # the Python class: point sizes, and a BN254-sized key is not taken for one of this curve
    with pytest.raises(ValueError, match="96 bytes"):
        pv.Bls12381VerifyingKey(ref.lib_vk(kd), G1[:64], g2)
    with pytest.raises(ValueError, match="384 bytes"):
        pv.Bls12381VerifyingKey(ref.lib_vk(kd), G1, g2[:256])


def test_batch_refusals():
    from gnark_amd import _lib
    _, kd, tau, pr, pub = instance(5, 2, 1)
    vk = lib_key(kd, tau)
    L, p = _lib.lib, _lib.ptr
    proof, wit, st = packed(pr), b"".join(o.fr_to_bytes(x) for x in pub), bytearray(1)
    none = _lib.HASH_FN()
    for fn in (L.gg_plonk_verify_batch_bls12_381, L.gg_plonk_verify_batch_bls12_381_host):
        for args, want in (((None, 1, p(proof), p(wit)), "null argument: vk"),
                           ((vk.handle, 0, p(proof), p(wit)), "n must be > 0"),
                           ((vk.handle, 1, None, p(wit)), "null argument: proofs"),
                           ((vk.handle, 1, p(proof), None), "null argument: public_witness")):
            assert fn(*args, none, None, none, None, p(st)) == 1
            assert want in L.gg_last_error().decode()
        assert fn(vk.handle, 1, p(proof), p(wit), none, None, none, None, None) == 1
        assert "null argument: status_out" in L.gg_last_error().decode()
    ok = bytearray(1)
    g2, pt, z = ref.g2_bytes(tau), G1, o.fr_to_bytes(3)
    for fn in (L.gg_kzg_verify_bls12_381, L.gg_kzg_verify_bls12_381_host):
        assert fn(0, p(G1), p(g2), p(pt), p(pt), p(z), p(z), p(ok)) == 1
        assert "n must be > 0" in L.gg_last_error().decode()
        assert fn(1, p(G1), p(g2), None, p(pt), p(z), p(z), p(ok)) == 1
        assert "null argument: digests" in L.gg_last_error().decode()
        assert fn(1, p(G1), p(g2[:192] + bytes(192)), p(pt), p(pt), p(z), p(z), p(ok)) == 1
        assert "kzg_g2[1] is the point at infinity" in L.gg_last_error().decode()
        assert fn(1, p(o.g1_to_bytes(g1_outside_subgroup())), p(g2), p(pt), p(pt), p(z), p(z), p(ok)) == 1
        assert "kzg_g1 is not in the r-torsion" in L.gg_last_error().decode()
    vk.close()

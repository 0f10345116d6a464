"""PlonK Verify and the KZG opening check on the host path
(gg_plonk_verify_batch_host, gg_kzg_verify_bn254_host: the per-proof functions
the kernels run, in a loop on the CPU) against the Python restatement of
verify.go (plonk_verify_ref.py) and the oracle's trapdoor verifier, on proofs
made by the oracle prover.  No GPU."""
import ctypes
import hashlib
import random

import pytest

import bn254_oracle as o
import plonk_prover_oracle as po
import plonk_verify_ref as ref
from pairing_ref import g1_off_curve, twist_point_outside_subgroup
from plonk_circuits import Circuit
from test_oracle_plonk_prover import blinding, oracle_key, oracle_solve

R = o.R
OK, MALFORMED, QUOTIENT, KZG = ref.OK, ref.MALFORMED, ref.QUOTIENT, ref.KZG
CASES = [(3, 0, 0), (4, 1, 0), (5, 2, 1), (5, 0, 2)]
_made = {}


def instance(log_n, nb_public, n_cmt, hashes=(None, None)):
    """(oracle key, key dict, tau, proof, public inputs), made once per case"""
    k = (log_n, nb_public, n_cmt, hashes)
    if k not in _made:
        circ = Circuit(log_n, 60 + log_n, nb_public=nb_public, n_cmt=n_cmt, curve="bn254")
        tau = random.Random(log_n + 1).randrange(2, R)
        key = oracle_key(circ, tau)
        L, Rv, O, pub, cmts = oracle_solve(circ, key, 11)
        pr = po.prove(key, L, Rv, O, pub, cmts, blinding(6, R), challenge_hash=hashes[0], folding_hash=hashes[1])
        _made[k] = (key, ref.key_dict(key), tau, pr, list(pub))
    return _made[k]


def lib_key(kd, tau):
    from gnark_amd import plonk_verify as pv
    return pv.VerifyingKey(ref.lib_vk(kd), o.g1_to_bytes(o.G1_GEN), ref.g2_bytes(tau))


def corruptions(pr, pub):
    """(name, proof, public inputs, expected status) of the (5, 2, 1) proof"""
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
    ]


def packed(pr):
    """the library's bytes of an oracle proof; a scalar >= r keeps its limbs"""
    from gnark_amd import plonk_prover as pp
    big = [j for j, v in enumerate(pr["claimed"]) if v >= R]
    q = dict(pr)
    q["claimed"] = [v % R for v in pr["claimed"]]
    b = bytearray(pp.proof_bytes(ref.lib_proof(q), "bn254"))
    nc = len(pr["bsb22"])
    for j in big:
        off = 64 * (8 + nc) + 32 * j
        b[off:off + 32] = pr["claimed"][j].to_bytes(32, "little")
    return bytes(b)


@pytest.mark.parametrize("log_n,nb_public,n_cmt", CASES)
def test_oracle_proofs_verify(log_n, nb_public, n_cmt):
    from gnark_amd import plonk_verify as pv
    key, kd, tau, pr, pub = instance(log_n, nb_public, n_cmt)
    vk = lib_key(kd, tau)
    assert vk.n_commitments == n_cmt
    assert pv.verify_batch([ref.lib_proof(pr)], vk, [pub], host=True) == [OK]
    pv.verify(ref.lib_proof(pr), vk, pub, host=True)
    assert ref.verify(kd, ref.g2_pair(tau), pr, pub) == OK
    assert po.verify_trapdoor(key, pr, pub)
    vk.close()


def test_every_corruption():
    from gnark_amd import plonk_verify as pv
    key, kd, tau, pr, pub = instance(5, 2, 1)
    vk = lib_key(kd, tau)
    cases = corruptions(pr, pub)
    got = pv.verify_batch([packed(q) for _, q, _, _ in cases] + [packed(pr)], vk,
                          [w for _, _, w, _ in cases] + [pub], host=True)
    assert got == [st for _, _, _, st in cases] + [OK]
    g2 = ref.g2_pair(tau)
    for name, q, w, st in cases:
        assert ref.verify(kd, g2, q, w) == st, name
        if st != MALFORMED:
            assert not po.verify_trapdoor(key, q, w), name
    with pytest.raises(pv.VerifyError, match="claimed quotient is not as expected") as e:
        pv.verify(packed(cases[0][1]), vk, pub, host=True)
    assert e.value.status == QUOTIENT
    with pytest.raises(pv.VerifyError, match="can't verify opening proof") as e:
        pv.verify(packed(cases[6][1]), vk, pub, host=True)
    assert e.value.status == KZG
    # a witness element >= r, by its limbs
    wit = o.fr_to_bytes(pub[0]) + R.to_bytes(32, "little")
    assert pv.verify_batch([packed(pr)], vk, [wit], host=True) == [MALFORMED]
    with pytest.raises(ValueError, match="invalid witness size"):
        pv.verify(packed(pr), vk, pub + [1], host=True)
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
    for pos, c in ((0, 6), (64, 0), (129, 7)):
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
        return o.g1_mul(G, po.horner(c, tau, R)) if po.horner(c, tau, R) else None

    def open_(c, z):
        y = po.horner(c, z, R)
        q = po._div_x_minus_a(c, y, z, R)
        return commit(c), (commit(q) if q else None), z, y
    z = rnd.randrange(R)
    good = open_(f, z)
    root = rnd.randrange(1, R)
    g = po._div_x_minus_a(f, po.horner(f, root, R), root, R)   # f = g (X - root) + f(root)
    vanishing = [(-c * root + d) % R for c, d in zip(g + [0], [0] + g)]  # g (X - root): y = 0 at root
    assert po.horner(vanishing, root, R) == 0
    return [good + (True,), (good[0], good[1], z, (good[3] + 1) % R, False), open_([5], z) + (True,),
            open_(f, 0) + (True,), open_(vanishing, root) + (True,)]


def test_kzg_verify_host():
    from gnark_amd import kzg
    tau = 0x1234567890abcdef1234567
    g2 = ref.g2_pair(tau)
    cases = kzg_cases(tau)
    assert cases[2][1] is None and cases[3][2] == 0 and cases[4][3] == 0
    b = o.g1_to_bytes
    got = kzg.verify(b(o.G1_GEN), ref.g2_bytes(tau), [b(c[0]) for c in cases], [b(c[1]) for c in cases],
                     [c[2] for c in cases], [c[3] for c in cases], host=True)
    assert got == [c[4] for c in cases]
    for c in cases:
        assert ref.kzg_check(g2, c[0], c[1], c[2], c[3]) == c[4]
    # a point off the curve is rejected by the check, not multiplied
    assert kzg.verify(b(o.G1_GEN), ref.g2_bytes(tau), [b(g1_off_curve(3))], [b(cases[0][1])], [1], [2],
                      host=True) == [False]


def _create(**over):
    """gg_plonk_vk_create on the (5, 2, 1) key with some arguments replaced -> (rc, message)"""
    from gnark_amd import _lib, fr
    _, kd, tau, _, _ = instance(5, 2, 1)
    b = o.g1_to_bytes
    a = dict(curve=_lib.GG_CURVE_BN254, size=kd["n"], generator=fr.fr_mont(kd["omega"]),
             coset_shift=fr.fr_mont(kd["u"]), S=b"".join(b(s) for s in kd["S"]),
             Q=b"".join(b(kd[q]) for q in ("Ql", "Qr", "Qm", "Qo", "Qk")), Qcp=b"".join(b(q) for q in kd["Qcp"]),
             n_cmt=1, idx=(ctypes.c_uint32 * 1)(*kd["cmt_idx"]), nb_public=kd["nb_public"], kzg_g1=b(o.G1_GEN),
             kzg_g2=ref.g2_bytes(tau))
    a.update(over)
    h = ctypes.c_void_p()
    p = _lib.ptr
    rc = _lib.lib.gg_plonk_vk_create(a["curve"], a["size"], p(a["generator"]), p(a["coset_shift"]), p(a["S"]),
                                     p(a["Q"]), p(a["Qcp"]), a["n_cmt"], a["idx"], a["nb_public"], p(a["kzg_g1"]),
                                     p(a["kzg_g2"]), ctypes.byref(h))
    msg = _lib.lib.gg_last_error().decode() if rc else ""
    if rc == 0:
        _lib.lib.gg_plonk_vk_destroy(h)
    return rc, msg


def test_key_refusals():
    from gnark_amd import _lib, plonk_verify as pv
    _, kd, tau, _, _ = instance(5, 2, 1)
    assert _create() == (0, "")
    for name in ("generator", "coset_shift", "S", "Q", "Qcp", "idx", "kzg_g1", "kzg_g2"):
        rc, msg = _create(**{name: None})
        want = "commitment_indexes" if name == "idx" else name
        assert rc == 1 and f"null argument: {want}" in msg, (name, msg)
    assert _lib.lib.gg_plonk_vk_create(0, 8, None, None, None, None, None, 0, None, 0, None, None, None) == 1
    assert "null argument: out" in _lib.lib.gg_last_error().decode()
    for size in (0, 1, 24):
        rc, msg = _create(size=size)
        assert rc == 1 and "power of two" in msg, msg
    rc, msg = _create(n_cmt=-1)
    assert rc == 1 and "n_cmt" in msg
    rc, msg = _create(idx=(ctypes.c_uint32 * 1)(kd["n"] - kd["nb_public"]))
    assert rc == 1 and "commitment index" in msg
    off = o.g1_to_bytes(g1_off_curve(9))
    good_s = b"".join(o.g1_to_bytes(s) for s in kd["S"])
    rc, msg = _create(S=good_s[:64] + off + good_s[128:])
    assert rc == 1 and "S[1] is not on the curve" in msg, msg
    rc, msg = _create(Qcp=off)
    assert rc == 1 and "Qcp[0] is not on the curve" in msg, msg
    rc, msg = _create(kzg_g1=off)
    assert rc == 1 and "kzg_g1 is not on the curve" in msg, msg
    g2 = ref.g2_bytes(tau)
    rc, msg = _create(kzg_g2=g2[:128] + bytes(128))
    assert rc == 1 and "kzg_g2[1] is the point at infinity" in msg, msg
    x, y = o.G2_GEN
    rc, msg = _create(kzg_g2=o.g2_to_bytes((x, y + o.Fp2(1, 0))) + g2[128:])
    assert rc == 1 and "kzg_g2[0] is not on the twist" in msg, msg
    rc, msg = _create(kzg_g2=g2[:128] + o.g2_to_bytes(twist_point_outside_subgroup(3)))
    assert rc == 1 and "kzg_g2[1] is not in the r-torsion" in msg, msg
    rc, msg = _create(curve=_lib.GG_CURVE_BLS12_381)
    assert rc == _lib.GG_ERR_UNSUPPORTED and "not supported" in msg
    with pytest.raises(ValueError, match="bn254"):
        pv.VerifyingKey(ref.lib_vk(kd), o.g1_to_bytes(o.G1_GEN), g2, curve="bls12-381")


def test_batch_refusals():
    from gnark_amd import _lib
    _, kd, tau, pr, pub = instance(5, 2, 1)
    vk = lib_key(kd, tau)
    L, p = _lib.lib, _lib.ptr
    proof, wit, st = packed(pr), b"".join(o.fr_to_bytes(x) for x in pub), bytearray(1)
    none = _lib.HASH_FN()
    for fn in (L.gg_plonk_verify_batch, L.gg_plonk_verify_batch_host):
        for args, want in (((None, 1, p(proof), p(wit)), "null argument: vk"),
                           ((vk.handle, 0, p(proof), p(wit)), "n must be > 0"),
                           ((vk.handle, 1, None, p(wit)), "null argument: proofs"),
                           ((vk.handle, 1, p(proof), None), "null argument: public_witness")):
            assert fn(*args, none, None, none, None, p(st)) == 1
            assert want in L.gg_last_error().decode()
        assert fn(vk.handle, 1, p(proof), p(wit), none, None, none, None, None) == 1
        assert "null argument: status_out" in L.gg_last_error().decode()
    ok = bytearray(1)
    g1, g2, pt, z = o.g1_to_bytes(o.G1_GEN), ref.g2_bytes(tau), o.g1_to_bytes(o.G1_GEN), o.fr_to_bytes(3)
    for fn in (L.gg_kzg_verify_bn254, L.gg_kzg_verify_bn254_host):
        assert fn(0, p(g1), p(g2), p(pt), p(pt), p(z), p(z), p(ok)) == 1
        assert "n must be > 0" in L.gg_last_error().decode()
        assert fn(1, p(g1), p(g2), None, p(pt), p(z), p(z), p(ok)) == 1
        assert "null argument: digests" in L.gg_last_error().decode()
        assert fn(1, p(g1), p(g2[:128] + bytes(128)), p(pt), p(pt), p(z), p(z), p(ok)) == 1
        assert "kzg_g2[1] is the point at infinity" in L.gg_last_error().decode()
    vk.close()

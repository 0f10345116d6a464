"""The pairing engine and Groth16 Verify, the parts that need no GPU: the same
templates the kernels run, on the host (gg_pairing_bn254_host), against the
oracle's pairing coefficient for coefficient; gg_hash_to_field_bn254 against
the BSB22 oracle; every refusal of gg_groth16_vk_create and
gg_groth16_verify_batch -- all decided on the host before the first device
call, so they answer on a machine without a GPU."""
import ctypes
from math import gcd

import numpy as np
import pytest

import bn254_oracle as o
import bn254_bsb22 as bo
import pairing_ref as pr


def _g1(p):
    return o.g1_to_bytes(p)


def _g2(q):
    return o.g2_to_bytes(q)


def test_gt_multiple_is_coprime_to_r():
    from gnark_amd import pairing
    x = o.BN_X
    assert pairing.GT_MULTIPLE == 2 * x * (6 * x * x + 3 * x + 1)
    assert gcd(pairing.GT_MULTIPLE, o.R) == 1
    assert pairing.GT_BYTES == 384 == len(pr.gt_one())


def test_e12_layout_roundtrip():
    f = o.Fp12([o.Fp2(2 * i + 1, 2 * i + 2) for i in range(6)])
    b = pr.gt_to_bytes(f)
    assert pr.gt_from_bytes(b) == f
    # C0.B1 (the second E2) is the w^2 coefficient, C1.B0 (the fourth) the w^1 coefficient
    assert o.fp_from_bytes(b[64:96]) == 5 and o.fp_from_bytes(b[192:224]) == 3


def test_host_pairing_of_the_generators():
    from gnark_amd import pairing
    got = pairing.pair(_g1(o.G1_GEN), _g2(o.G2_GEN), host=True)[0]
    assert got == pr.gt_to_bytes(pr.e_gen() ** pairing.GT_MULTIPLE)


def test_host_pairing_random_pairs_and_product():
    """three random pairs one by one, then their product with k = 3 (one
    squaring shared by the three Miller loops)"""
    from gnark_amd import pairing
    rng = o.SplitMix64(2024)
    ps = [o.g1_mul(o.G1_GEN, rng.fr()) for _ in range(3)]
    qs = [o.g2_mul(o.G2_GEN, rng.fr()) for _ in range(3)]
    g1 = b"".join(_g1(p) for p in ps)
    g2 = b"".join(_g2(q) for q in qs)
    want = [o.pairing(p, q) ** pairing.GT_MULTIPLE for p, q in zip(ps, qs)]
    got = pairing.pair(g1, g2, k=1, host=True)
    assert got == [pr.gt_to_bytes(w) for w in want]
    prod = pairing.pair(g1, g2, k=3, host=True)
    assert prod == [pr.gt_to_bytes(want[0] * want[1] * want[2])]


def test_host_pairing_infinity_contributes_one():
    from gnark_amd import pairing
    p, q = o.g1_mul(o.G1_GEN, 11), o.g2_mul(o.G2_GEN, 13)
    one = pr.gt_one()
    assert pairing.pair(bytes(64), _g2(q), host=True) == [one]
    assert pairing.pair(_g1(p), bytes(128), host=True) == [one]
    # inside a product: e(P, Q) * e(inf, Q) * e(P, inf) = e(P, Q); e(G1, G2)^(11 * 13 * m)
    got = pairing.pair(_g1(p) + bytes(64) + _g1(p), _g2(q) + _g2(q) + bytes(128), k=3, host=True)
    assert got == [pr.e_power(11 * 13, pairing.GT_MULTIPLE)]
    # k = 4: a chunk of three pairs and a chunk of one; e(P, Q)^2 e(-P, Q) e(P, Q) = e(P, Q)^2
    np_ = (p[0], (-p[1]) % o.P)
    got = pairing.pair(_g1(p) * 2 + _g1(np_) + _g1(p), _g2(q) * 4, k=4, host=True)
    assert got == [pr.e_power(2 * 11 * 13, pairing.GT_MULTIPLE)]


def test_pairing_argument_refusals():
    from gnark_amd._lib import lib, ptr
    out = bytearray(384)
    g1, g2 = _g1(o.G1_GEN), _g2(o.G2_GEN)
    for fn in (lib.gg_pairing_bn254_host, lib.gg_pairing_bn254):
        for args, name in (((0, 1, ptr(g1), ptr(g2), ptr(out)), "n must be"), ((1, 0, ptr(g1), ptr(g2), ptr(out)), "k must be"),
                           ((1, 1, None, ptr(g2), ptr(out)), "g1"), ((1, 1, ptr(g1), None, ptr(out)), "g2"),
                           ((1, 1, ptr(g1), ptr(g2), None), "gt_out")):
            assert fn(*args) == 1
            assert name in lib.gg_last_error().decode()
    assert lib.gg_g2_check_bn254(0, ptr(g2), ptr(out)) == 1 and "n must be" in lib.gg_last_error().decode()
    assert lib.gg_g1_check_bn254(1, None, ptr(out)) == 1 and "g1" in lib.gg_last_error().decode()


def test_hash_to_field_matches_oracle():
    from gnark_amd import pairing
    rcs, cinfo = bo.bsb22_test_circuit(1)
    # the commitment prehash of the one-commitment circuit: Marshal(C) | the public committed value X
    c = o.g1_mul(o.G1_GEN, 0xC0FFEE)
    msg = o.g1_raw_encode(c) + (7).to_bytes(32, "big")
    assert len(cinfo[0].public_committed) == 1 and len(msg) == 96
    for m in (msg, b"", bytes(range(256)) + bytes(44)):
        assert o.fr_from_bytes(pairing.hash_to_field(m)) == bo.hash_to_field(m), len(m)
    assert o.fr_from_bytes(pairing.hash_to_field(msg)) == bo.commitment_hash(c, [7])
    assert o.fr_from_bytes(pairing.hash_to_field(b"abc", b"QUUX-V01-CS02-with-expander-SHA256-128")) == \
        bo.hash_to_field(b"abc", b"QUUX-V01-CS02-with-expander-SHA256-128")


# ------------------------------------------------------------ refusals of gg_groth16_vk_create
class _Key:
    """A valid call of gg_groth16_vk_create (nb_public 3, one commitment) whose
    fields the cases break one at a time.  No case reaches the device."""

    def __init__(self):
        self.curve = 0
        self.g1 = _g1(o.G1_GEN)
        self.g2 = _g2(o.G2_GEN)
        self.nb_public, self.nc, self.n_K = 3, 1, 4
        self.off, self.idx = [0, 2], [1, 2]
        self.null = None
        self.no_out = False

    def call(self):
        from gnark_amd._lib import lib, ptr
        K = self.g1 * max(1, self.n_K)
        off = np.array(self.off, np.uint32)
        idx = np.array(self.idx, np.uint32)
        args = dict(alpha1=ptr(self.g1), beta2=ptr(self.g2), gamma2=ptr(self.g2), delta2=ptr(self.g2), K=ptr(K),
                    ped_g=ptr(self.g2), ped_g_root_sigma_neg=ptr(self.g2), committed_off=ptr(off),
                    committed_idx=ptr(idx))
        if self.null:
            args[self.null] = None
        h = ctypes.c_void_p()
        rc = lib.gg_groth16_vk_create(self.curve, args["alpha1"], args["beta2"], args["gamma2"], args["delta2"],
                                      args["K"], self.n_K, self.nb_public, args["ped_g"],
                                      args["ped_g_root_sigma_neg"], args["committed_off"], args["committed_idx"],
                                      self.nc, None if self.no_out else ctypes.byref(h))
        assert h.value is None
        return rc, lib.gg_last_error().decode()


@pytest.mark.parametrize("name", ["alpha1", "beta2", "gamma2", "delta2", "K", "ped_g", "ped_g_root_sigma_neg",
                                  "committed_off", "committed_idx", "out"])
def test_vk_create_refuses_null_pointers(name):
    k = _Key()
    if name == "out":
        k.no_out = True
    else:
        k.null = name
    rc, msg = k.call()
    assert rc == 1 and "null argument" in msg and name in msg, (rc, msg)


def test_vk_create_refusals_name_the_offender():
    k = _Key()
    k.nb_public, k.n_K = 0, 1
    rc, msg = k.call()
    assert rc == 1 and "nb_public" in msg
    k = _Key()
    k.n_K = 5
    rc, msg = k.call()
    assert rc == 1 and "n_K = 5" in msg and "nb_public + n_commitments = 4" in msg
    k = _Key()
    k.nb_public, k.n_K = 1030, 1031
    rc, msg = k.call()
    assert rc == 1 and "GG_VERIFY_MAX_K" in msg
    k = _Key()
    k.nc, k.n_K = -1, 2
    rc, msg = k.call()
    assert rc == 1 and "n_commitments" in msg
    for bad in (0, 3, 77):     # commitment 0 may commit to the public inputs 1 .. nb_public - 1 only
        k = _Key()
        k.idx = [1, bad]
        rc, msg = k.call()
        assert rc == 1 and f"committed index {bad}" in msg and "commitment 0" in msg, msg
    k = _Key()
    k.off = [1, 2]
    rc, msg = k.call()
    assert rc == 1 and "committed_off" in msg
    k = _Key()
    k.g2 = bytes(128)
    rc, msg = k.call()
    assert rc == 1 and "infinity" in msg


@pytest.mark.parametrize("curve", [1, 7])
def test_vk_create_refuses_other_curves(curve):
    from gnark_amd._lib import GG_ERR_UNSUPPORTED
    k = _Key()
    k.curve = curve
    rc, msg = k.call()
    assert rc == GG_ERR_UNSUPPORTED and "BN254" in msg and f"curve {curve}" in msg


def test_verifying_key_class_refuses_bls12_381():
    from gnark_amd import groth16
    from gnark_amd._lib import GnarkAmdError
    d = groth16.VerifyingKeyData(alpha1=bytes(96), beta1=bytes(96), delta1=bytes(96), beta2=bytes(192),
                                 gamma2=bytes(192), delta2=bytes(192), K=bytes(96 * 2), nb_public=2,
                                 curve="bls12-381")
    with pytest.raises(GnarkAmdError) as e:
        groth16.VerifyingKey(d)
    assert e.value.code == 4 and "BN254" in str(e.value)


def test_verify_batch_refusals():
    """vk NULL, n = 0 and the null arrays are refused before the key is looked at"""
    from gnark_amd._lib import lib, ptr
    buf = bytearray(256)
    st = bytearray(1)
    rc = lib.gg_groth16_verify_batch(None, 1, ptr(buf), None, None, ptr(buf), ptr(st))
    assert rc == 1 and "vk" in lib.gg_last_error().decode()
    fake = ctypes.c_void_p(8)   # never dereferenced: the counts and pointers are checked first
    rc = lib.gg_groth16_verify_batch(fake, 0, ptr(buf), None, None, ptr(buf), ptr(st))
    assert rc == 1 and "n must be" in lib.gg_last_error().decode()
    rc = lib.gg_groth16_verify_batch(fake, 1, None, None, None, ptr(buf), ptr(st))
    assert rc == 1 and "proofs" in lib.gg_last_error().decode()
    rc = lib.gg_groth16_verify_batch(fake, 1, ptr(buf), None, None, ptr(buf), None)
    assert rc == 1 and "status_out" in lib.gg_last_error().decode()
    rc = lib.gg_groth16_verify_batch(fake, (1 << 24) + 1, ptr(buf), None, None, ptr(buf), ptr(st))
    assert rc == 1 and "2^24" in lib.gg_last_error().decode()

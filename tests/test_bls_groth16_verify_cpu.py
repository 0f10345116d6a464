"""Groth16 Verify over BLS12-381, the parts that need no GPU: the exports, every
refusal of gg_groth16_vk_create_bls12_381 (decided on the host; the key makes no
device call), gg_hash_to_field_bls12_381 against the oracle, and the host run of
the verifier's per-proof functions (verify_batch(..., host=True)) on the
reference's twelve bellman vectors and on a synthetic BSB22 key.  The host run
uses the endomorphism subgroup checks the kernels use."""
import ctypes

import numpy as np
import pytest

import bls12_381_oracle as o
import bls_groth16_ref as gr
import bls_pairing_ref as br

OK, SUBGROUP, PEDERSEN, PAIRING = gr.OK, gr.SUBGROUP, gr.PEDERSEN, gr.PAIRING
SYMBOLS = ["gg_groth16_vk_create_bls12_381", "gg_groth16_vk_destroy_bls12_381", "gg_groth16_verify_batch_bls12_381",
           "gg_groth16_verify_batch_bls12_381_host", "gg_hash_to_field_bls12_381", "gg_g1_check_endo_bls12_381",
           "gg_g2_check_endo_bls12_381"]


def test_the_seven_symbols_are_exported():
    from gnark_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and getattr(_lib.lib, name) is not None, name
    from gnark_amd import groth16
    assert groth16.Bls12381VerifyingKey.curve == "bls12-381"


def test_endomorphism_constants_in_the_header_are_the_generators():
    """BETA and PSI of Bls12381Tower are what tools/gen_bls12_381_tower.py --endo derives
    (it asserts [x^2] phi(G1) + G1 = 0 and psi(G2) = [x] G2 while it runs)"""
    import contextlib
    import importlib.util
    import io
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_bls12_381_tower",
                                                  os.path.join(root, "tools", "gen_bls12_381_tower.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tool.main_endo()
    tables = out.getvalue()
    assert tables.count("0x") == 12 + 2 * 24
    assert tables in open(os.path.join(root, "gnark-fork_amd", "csrc", "pairing.cuh")).read()
    # phi acts as x^2 - 1 on G1 and psi as x on G2
    x = tool.X
    beta = tool.endo_beta()
    assert (beta * o.G1_GEN[0] % o.P, o.G1_GEN[1]) == o.g1_mul(o.G1_GEN, (x * x - 1) % o.R)
    cx, cy = tool.endo_psi()
    conj = lambda a: (a[0], -a[1] % o.P)
    q = o.g2_mul(o.G2_GEN, 0xFEEDFACE)
    assert (o.f2_mul(conj(q[0]), cx), o.f2_mul(conj(q[1]), cy)) == o.g2_mul(q, x % o.R)


# ------------------------------------------------------------ refusals of gg_groth16_vk_create_bls12_381
class _Key:
    """A valid call of gg_groth16_vk_create_bls12_381 (nb_public 3, one commitment)
    whose fields the cases break one at a time."""

    def __init__(self):
        self.g1 = o.g1_to_bytes(o.G1_GEN)
        self.g2 = o.g2_to_bytes(o.G2_GEN)
        self.nb_public, self.nc, self.n_K = 3, 1, 4
        self.off, self.idx = [0, 2], [1, 2]
        self.null = None
        self.no_out = False

    def call(self, expect_handle=False):
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
        rc = lib.gg_groth16_vk_create_bls12_381(args["alpha1"], args["beta2"], args["gamma2"], args["delta2"],
                                                args["K"], self.n_K, self.nb_public, args["ped_g"],
                                                args["ped_g_root_sigma_neg"], args["committed_off"],
                                                args["committed_idx"], self.nc,
                                                None if self.no_out else ctypes.byref(h))
        msg = lib.gg_last_error().decode()
        if expect_handle:
            assert rc == 0 and h.value, (rc, msg)
            assert lib.gg_groth16_vk_destroy_bls12_381(h) == 0
        else:
            assert h.value is None
        return rc, msg


def test_vk_create_accepts_the_unbroken_call():
    assert _Key().call(expect_handle=True)[0] == 0


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
    k.g2 = bytes(192)
    rc, msg = k.call()
    assert rc == 1 and "infinity" in msg


@pytest.mark.parametrize("host", [True, False])
def test_verify_batch_refusals(host):
    """vk NULL, n = 0 and the null arrays are refused before the key is looked at"""
    from gnark_amd._lib import lib, ptr
    fn = lib.gg_groth16_verify_batch_bls12_381_host if host else lib.gg_groth16_verify_batch_bls12_381
    buf = bytearray(384)
    st = bytearray(1)
    assert fn(None, 1, ptr(buf), None, None, ptr(buf), ptr(st)) == 1 and "vk" in lib.gg_last_error().decode()
    fake = ctypes.c_void_p(8)   # never dereferenced: the counts and pointers are checked first
    assert fn(fake, 0, ptr(buf), None, None, ptr(buf), ptr(st)) == 1 and "n must be" in lib.gg_last_error().decode()
    assert fn(fake, 1, None, None, None, ptr(buf), ptr(st)) == 1 and "proofs" in lib.gg_last_error().decode()
    assert fn(fake, 1, ptr(buf), None, None, ptr(buf), None) == 1 and "status_out" in lib.gg_last_error().decode()
    assert fn(fake, (1 << 24) + 1, ptr(buf), None, None, ptr(buf), ptr(st)) == 1
    assert "2^24" in lib.gg_last_error().decode()


def test_verify_batch_refuses_missing_arrays_of_a_key_with_commitments():
    from gnark_amd import groth16
    from gnark_amd._lib import lib, ptr
    key = gr.SyntheticKey(1, seed=5, nc=1)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    buf, st = bytearray(384), bytearray(1)
    fn = lib.gg_groth16_verify_batch_bls12_381_host
    assert fn(vk.handle, 1, ptr(buf), None, ptr(buf), ptr(buf), ptr(st)) == 1
    assert "commitments" in lib.gg_last_error().decode()
    assert fn(vk.handle, 1, ptr(buf), ptr(buf), None, ptr(buf), ptr(st)) == 1 and "poks" in lib.gg_last_error().decode()
    assert fn(vk.handle, 1, ptr(buf), ptr(buf), ptr(buf), None, ptr(st)) == 1
    assert "public_witness" in lib.gg_last_error().decode()
    vk.close()


def test_python_refusals():
    from gnark_amd import groth16
    import bn254_oracle as bn
    d = gr.SyntheticKey(0, seed=1).vk_data()
    d.curve = "bn254"
    with pytest.raises(ValueError, match="bls12-381"):
        groth16.Bls12381VerifyingKey(d)
    key = gr.SyntheticKey(1, seed=2)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    assert (vk.n_commitments, vk.nb_public) == (0, 2)
    p = key.prove([5]).gproof()
    with pytest.raises(ValueError, match="invalid witness size, got 2, expected 1"):
        groth16.verify_batch([p], vk, [[5, 6]], host=True)
    with pytest.raises(ValueError, match="1 proofs, 2 witnesses"):
        groth16.verify_batch([p], vk, [[5], [5]], host=True)
    short = groth16.Proof(bn.g1_to_bytes(bn.G1_GEN), bn.g2_to_bytes(bn.G2_GEN), bn.g1_to_bytes(bn.G1_GEN))
    with pytest.raises(ValueError, match="96-byte G1"):
        groth16.verify_batch([short], vk, [[5]], host=True)
    vk.close()

    class _Bn254Key:     # host=True is refused before a BN254 key is used
        n_commitments, nb_public = 0, 1
    with pytest.raises(ValueError, match="host=True"):
        groth16.verify_batch([], _Bn254Key(), [], host=True)


# ------------------------------------------------------------ hash_to_field
def test_hash_to_field_matches_oracle():
    from gnark_amd import pairing
    c = o.g1_mul(o.G1_GEN, 0xC0FFEE)
    short = o.g1_raw_bytes(c) + (7).to_bytes(32, "big")
    for m in (b"", short, bytes(range(256)) + bytes(44)):
        got = pairing.hash_to_field(m, curve="bls12-381")
        assert o.fr_from_bytes(got) == o.hash_to_field(m, b"bsb22-commitment"), len(m)
    assert len(short) == 128 and o.fr_from_bytes(pairing.hash_to_field(short, curve="bls12-381")) == \
        gr.commitment_hash(c, [7])
    assert o.fr_from_bytes(pairing.hash_to_field(b"abc", b"QUUX-V01-CS02", curve="bls12-381")) == \
        o.hash_to_field(b"abc", b"QUUX-V01-CS02")


# ------------------------------------------------------------ the host verifier
def test_bellman_vectors_on_the_host():
    cases = br.load_bellman_kats()
    want = [OK if c["ok"] else PAIRING for c in cases]
    assert len(cases) == 12 and want.count(OK) == 6 and want.count(PAIRING) == 6
    assert gr.kat_statuses(cases, host=True) == want


def test_bellman_vectors_under_one_key_in_one_batch():
    """the vectors that share the first vector's key, as one batch"""
    from gnark_amd import groth16
    cases = br.load_bellman_kats()
    key = gr.kat_vk_data(cases[0])
    same = [c for c in cases if gr.kat_vk_data(c) == key]
    vk = groth16.Bls12381VerifyingKey(key)
    got = groth16.verify_batch([gr.kat_proof(c).gproof() for c in same], vk, [c["inputs"] for c in same], host=True)
    assert got == [OK if c["ok"] else PAIRING for c in same]
    vk.close()


def test_synthetic_bsb22_key_on_the_host():
    from gnark_amd import groth16
    key = gr.SyntheticKey(3, seed=31, nc=2)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    assert (vk.n_commitments, vk.nb_public) == (2, 4)
    wit = [11, 0, o.R - 1]
    p = key.prove(wit)
    outside = br.g1_outside_subgroup()
    flipped = [11, 1, o.R - 1]          # input 2 is not committed: the hashes and the Pedersen check stay
    cases = [(p, wit, OK),
             (p.replace(pok=o.g1_add(p.pok, o.G1_GEN)), wit, PEDERSEN),
             (p.replace(ar=br.g1_off_curve(7)), wit, SUBGROUP),
             (p.replace(krs=outside), wit, SUBGROUP),
             (p, flipped, PAIRING)]
    got = groth16.verify_batch([q.gproof() for q, _, _ in cases], vk, [w for _, w, _ in cases], host=True)
    assert got == [st for _, _, st in cases]
    groth16.verify(p.gproof(), vk, wit, host=True)
    with pytest.raises(groth16.VerifyError, match="pairing doesn't match") as e:
        groth16.verify(p.gproof(), vk, flipped, host=True)
    assert e.value.status == PAIRING
    # fr Montgomery bytes in place of integers
    assert groth16.verify_batch([p.gproof()], vk, [o.fr_vec_to_bytes(wit)], host=True) == [OK]
    vk.close()


def test_unused_public_input_on_the_host():
    """K[2] at infinity: whatever the dead input is, it adds nothing to kSum"""
    from gnark_amd import groth16
    key, proofs, wits, want = gr.unused_input_case()
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    assert groth16.verify_batch([p.gproof() for p in proofs], vk, wits, host=True) == want == [OK, OK, OK, PAIRING]
    vk.close()


@pytest.mark.parametrize("nb_inputs", [0, 1])
def test_synthetic_keys_without_commitments_on_the_host(nb_inputs):
    from gnark_amd import groth16
    key = gr.SyntheticKey(nb_inputs, seed=40 + nb_inputs)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    wit = [o.R - 1][:nb_inputs]
    p = key.prove(wit)
    bs_outside = p.replace(bs=br.twist_point_outside_subgroup(3))
    got = groth16.verify_batch([p.gproof(), bs_outside.gproof(), p.replace(krs=o.G1_GEN).gproof()], vk, [wit] * 3,
                               host=True)
    assert got == [OK, SUBGROUP, PAIRING]
    # the infinity is a member: Ar at infinity passes the point checks and fails the equation
    assert groth16.verify_batch([p.replace(ar=o.INF).gproof()], vk, [wit], host=True) == [PAIRING]
    vk.close()

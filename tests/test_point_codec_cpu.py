"""gnark-crypto's point codec on the host (gg_points_decode_host,
gg_points_encode_host, gg_fp_sqrt_host: the per-point code of the kernels, run on
the calling thread) against the Python codecs the project already has, and the
key / proof readers and writers built on it (gnark_amd.pkio) against the
bellman vectors of bellman_test.go.  No GPU."""
import base64
import json
import os

import pytest

import bls12_381_oracle as bls
import bls_pairing_ref as bref
import point_codec_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- 1. square roots
@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
@pytest.mark.parametrize("degree", [1, 2])
def test_fp_sqrt_host(curve, degree):
    from gnark_amd import codec
    data, vals, ok = ref.sqrt_inputs(curve, degree)
    roots, got = codec.fp_sqrt(data, curve, degree, host=True)
    assert list(got) == ok
    assert 0 < sum(ok) < len(ok)
    p = ref.bn.P if curve == "bn254" else bls.P
    fb = 32 if curve == "bn254" else 48
    for i, a in enumerate(vals):
        if not ok[i]:
            continue
        r = [ref.unmont(roots[(i * degree + k) * fb:(i * degree + k + 1) * fb], curve) for k in range(degree)]
        if degree == 1:
            assert r[0] * r[0] % p == a, i
        else:
            assert ref.f2_mul(r, r, p) == a, i
    if degree == 2:  # -1 = u^2: the purely imaginary branch
        r = [ref.unmont(roots[(4 + k) * fb:(5 + k) * fb], curve) for k in range(2)]
        assert r[0] == 0 and r[1] in (1, p - 1)


# ---------------------------------------------------------------- 2. against the reference codecs
@pytest.mark.parametrize("name", ref.GROUP_NAMES)
@pytest.mark.parametrize("raw", [False, True])
def test_decode_and_encode_match_the_reference(name, raw):
    from gnark_amd import codec
    g = ref.group(name)
    mont, enc = ref.encoded(name, raw, 65)
    assert mont[:g.pt] == bytes(g.pt) and mont[64 * g.pt:] == bytes(g.pt)  # the infinity at 0 and 64
    assert codec.encoded_size(g.gid, raw) == g.esz(raw) and len(enc) == 65 * g.esz(raw)
    pts, status = codec.decode_statuses(enc, g.gid, 65, raw=raw, host=True)
    assert status == bytes(65)
    assert pts == mont
    assert codec.decode_points(enc, g.gid, 65, raw=raw, subgroup_check=False, host=True) == mont
    assert codec.encode_points(mont, g.gid, raw=raw, host=True) == enc


# ---------------------------------------------------------------- 3. statuses
@pytest.mark.parametrize("name", ref.GROUP_NAMES)
def test_statuses(name):
    from gnark_amd import codec
    g = ref.group(name)
    cases = ref.bad_cases(name)
    labels = [c[0] for c in cases]
    assert any("no y" in s for s in labels) and any("y + 1" in s for s in labels)
    assert any("subgroup" in s for s in labels) == (name != "bn254-g1")
    for label, raw, blob, st_checked, st_unsafe, value in cases:
        assert len(blob) == g.esz(raw), label
        mont, enc = ref.encoded(name, raw, 3)
        good1, good2 = enc[g.esz(raw):2 * g.esz(raw)], enc[2 * g.esz(raw):]
        pts, status = codec.decode_statuses(good1 + blob + good2, g.gid, 3, raw=raw, host=True)
        assert list(status) == [0, st_checked, 0], label
        # a point that is not OK is the infinity; its neighbours keep their values
        assert pts == mont[g.pt:2 * g.pt] + bytes(g.pt) + mont[2 * g.pt:], label
        with pytest.raises(ValueError, match=f"point 1: .*status {st_checked}"):
            codec.decode_points(good1 + blob + good2, g.gid, 3, raw=raw, host=True)
        if st_unsafe is not None:
            pts, status = codec.decode_statuses(good1 + blob + good2, g.gid, 3, raw=raw, subgroup_check=False,
                                                host=True)
            assert list(status) == [0, st_unsafe, 0], label
            if value is not None:
                assert pts[g.pt:2 * g.pt] == value, label


def test_entry_points_refuse_bad_arguments():
    from gnark_amd import GnarkAmdError, _lib, codec
    assert _lib.lib.gg_point_encoded_size(9, 0) == 0 and _lib.lib.gg_point_encoded_size(_lib.GG_G1, 2) == 0
    st, out = bytearray(1), bytearray(64)
    rc = _lib.lib.gg_points_decode_host(7, 0, 0, 1, _lib.ptr(bytes(32)), _lib.ptr(out), _lib.ptr(st))
    assert rc == 1 and b"group" in _lib.lib.gg_last_error()
    rc = _lib.lib.gg_points_decode_host(_lib.GG_G1, 0, 2, 1, _lib.ptr(bytes(32)), _lib.ptr(out), _lib.ptr(st))
    assert rc == 1 and b"flags" in _lib.lib.gg_last_error()
    rc = _lib.lib.gg_fp_sqrt_host(0, 3, 1, _lib.ptr(bytes(32)), _lib.ptr(out), _lib.ptr(st))
    assert rc == 1 and b"degree" in _lib.lib.gg_last_error()
    with pytest.raises(ValueError):
        codec.decode_points(bytes(31), _lib.GG_G1, 1, host=True)
    with pytest.raises(GnarkAmdError):
        _lib.check(_lib.lib.gg_points_encode_host(_lib.GG_G1, 0, 1, None, _lib.ptr(out)))


# ---------------------------------------------------------------- 4. the bellman vectors
def _blobs():
    with open(os.path.join(HERE, "golden", "bls12_381_groth16_kats.json")) as fh:
        return [tuple(base64.b64decode(c[k]) for k in ("vk", "proof")) for c in json.load(fh)["cases"]]


def check_bellman_vectors(codec_name, host_verify):
    """shared with test_gpu_point_codec.py"""
    from gnark_amd import groth16, pkio
    kats = bref.load_bellman_kats()
    blobs = _blobs()
    assert len(kats) == len(blobs) == 12
    verdicts = []
    for kat, (vkb, proofb) in zip(kats, blobs):
        vk = pkio.read_verifying_key(vkb, curve="bls12-381", codec=codec_name)
        assert (vk.alpha1, vk.beta2, vk.gamma2, vk.delta2) == (
            bls.g1_to_bytes(kat["alpha"]), bls.g2_to_bytes(kat["beta"]), bls.g2_to_bytes(kat["gamma"]),
            bls.g2_to_bytes(kat["delta"]))
        assert vk.K == b"".join(bls.g1_to_bytes(p) for p in kat["K"])
        assert vk.nb_public == len(kat["K"]) and vk.commitment_key_g is None
        assert list(vk.public_and_commitment_committed) == [] and vk.curve == "bls12-381"
        assert pkio.write_verifying_key(vk, codec=codec_name) == vkb
        # bellman_test.go:101: no commitments (u32 0) and a raw all-zero CommitmentPok
        proof = pkio.read_proof(proofb + bytes(96 + 4), curve="bls12-381", codec=codec_name)
        assert (proof.Ar, proof.Bs, proof.Krs) == (
            bls.g1_to_bytes(kat["ar"]), bls.g2_to_bytes(kat["bs"]), bls.g1_to_bytes(kat["krs"]))
        assert proof.Commitments == () and proof.CommitmentPok == bytes(96)
        assert pkio.write_proof(proof, curve="bls12-381", codec=codec_name)[:192] == proofb
        key = groth16.Bls12381VerifyingKey(vk)
        try:
            verdicts.append(groth16.verify_batch([proof], key, [kat["inputs"]], host=host_verify)[0] == 0)
        finally:
            key.close()
    assert verdicts == [k["ok"] for k in kats]
    assert any(verdicts) and not all(verdicts)


def test_bellman_vectors_host():
    check_bellman_vectors("host", True)


# ---------------------------------------------------------------- 5. proving-key round trips
def test_proving_key_roundtrip_bn254():
    from gnark_amd import pkio
    from test_pkio import _data
    _, d = _data(1)
    cks = [(d.g1_A[:128], d.g1_B[:64])]
    for raw in (False, True):
        blob = pkio.write_proving_key(d, raw=raw, commitment_keys=cks)
        back, cks2 = pkio.read_proving_key(blob, nb_public=d.nb_public, codec="host")
        assert cks2 == cks
        assert pkio.write_proving_key(back, raw=raw, commitment_keys=cks2, codec="host") == blob
        ref_back, ref_cks = pkio.read_proving_key(blob, nb_public=d.nb_public, codec="python")
        assert back == ref_back and cks2 == ref_cks
        assert pkio.read_proving_key(blob, nb_public=d.nb_public, codec="host", unsafe=True)[0] == ref_back


def test_proving_key_reader_names_the_bad_point():
    from gnark_amd import pkio
    from test_pkio import _data
    _, d = _data(1)
    blob = bytearray(pkio.write_proving_key(d, raw=True))
    off = 168 + 3 * 64 + 4 + 5 * 64  # G1.A[5]
    blob[off + 63] ^= 1
    with pytest.raises(ValueError, match=r"pk: G1\.A: point 5: not on the curve"):
        pkio.read_proving_key(bytes(blob), nb_public=d.nb_public, codec="host")
    with pytest.raises(ValueError):
        pkio.read_proving_key(bytes(blob[:400]), nb_public=d.nb_public, codec="host")
    with pytest.raises(ValueError, match="BN254 only"):
        pkio.read_proving_key(bytes(blob), nb_public=d.nb_public, curve="bls12-381")


def test_verifying_key_and_proof_roundtrip_bn254():
    """A BN254 key with one commitment and a proof with one, through every codec."""
    from gnark_amd import groth16, pkio
    mont, _ = ref.encoded("bn254-g1", False, 12)
    g2, _ = ref.encoded("bn254-g2", False, 8)
    p1 = [mont[64 * i:64 * i + 64] for i in range(1, 12)]
    p2 = [g2[128 * i:128 * i + 128] for i in range(1, 8)]
    vk = groth16.VerifyingKeyData(alpha1=p1[0], beta1=p1[1], delta1=p1[2], beta2=p2[0], gamma2=p2[1], delta2=p2[2],
                                  K=b"".join(p1[3:9]), nb_public=5, commitment_key_g=p2[3],
                                  commitment_key_g_root_sigma_neg=p2[4], public_and_commitment_committed=[[1, 3]])
    proof = groth16.Proof(Ar=p1[9], Bs=p2[5], Krs=p1[10], Commitments=(p1[4],), CommitmentPok=p1[5])
    for raw in (False, True):
        vkb = pkio.write_verifying_key(vk, raw=raw)
        pb = pkio.write_proof(proof, raw=raw)
        if raw:
            assert pb == proof.write_raw()
        for c in ("python", "host"):
            assert pkio.write_verifying_key(vk, raw=raw, codec=c) == vkb
            assert pkio.read_verifying_key(vkb, codec=c) == vk
            assert pkio.write_proof(proof, raw=raw, codec=c) == pb
            assert pkio.read_proof(pb, codec=c) == proof
    n_g1 = 3 + 6
    assert len(pkio.write_verifying_key(vk)) == 32 * n_g1 + 64 * 3 + 4 + (4 + 4 + 16) + 2 * 64

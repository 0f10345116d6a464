"""The point codec kernels (gg_points_decode, gg_points_encode, gg_fp_sqrt)
against the host path of the same source, byte for byte, and the key / proof
readers with codec="gpu": the bellman vectors through the GPU verifier, and keys
made by the GPU setup, written compressed, read back on the GPU and proved with."""
import random

import pytest

import bn254_bsb22 as bo
import bn254_oracle as o
import point_codec_ref as ref
import r1cs_solver
from test_point_codec_cpu import check_bellman_vectors

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # wave and block edges; with GG_CODEC_CHUNK = 128 the chunk loop and its tail


@pytest.fixture(params=[None, "128"], ids=["chunk-default", "chunk-128"])
def chunk(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("GG_CODEC_CHUNK", raising=False)
    else:
        monkeypatch.setenv("GG_CODEC_CHUNK", request.param)  # read by the library at every call
    return request.param


# ---------------------------------------------------------------- 6. GPU against host
@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
@pytest.mark.parametrize("degree", [1, 2])
def test_fp_sqrt_gpu_equals_host(curve, degree, chunk):
    from gnark_amd import _lib, codec
    data, _, ok = ref.sqrt_inputs(curve, degree)
    want = codec.fp_sqrt(data, curve, degree, host=True)
    assert list(want[1]) == ok
    assert codec.fp_sqrt(data, curve, degree) == want
    # device operands and results
    n = len(ok)
    din, dout, dok = _lib.DeviceBuffer.from_host(data), _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(n)
    _lib.check(_lib.lib.gg_fp_sqrt(_lib.GG_CURVE_BN254 if curve == "bn254" else _lib.GG_CURVE_BLS12_381, degree, n,
                                   _lib.ptr(din), _lib.ptr(dout), _lib.ptr(dok)))
    assert (dout.to_host(), dok.to_host()) == want


@pytest.mark.parametrize("name", ref.GROUP_NAMES)
@pytest.mark.parametrize("raw", [False, True], ids=["compressed", "raw"])
def test_decode_and_encode_gpu_equal_host(name, raw, chunk):
    from gnark_amd import _lib, codec
    g = ref.group(name)
    for n in SIZES:
        mont, enc = ref.encoded(name, raw, n + 1)
        if n == 1:  # a finite point, not the infinity at index 0
            mont, enc = mont[g.pt:], enc[g.esz(raw):]
        else:
            mont, enc = mont[:n * g.pt], enc[:n * g.esz(raw)]
        n_eff = n
        want = codec.decode_statuses(enc, g.gid, n_eff, raw=raw, host=True)
        assert want == (mont, bytes(n_eff))
        assert codec.decode_statuses(enc, g.gid, n_eff, raw=raw) == want
        assert codec.encode_points(mont, g.gid, raw=raw) == enc
        # device bytes in, device points out; device points in
        dbuf = _lib.DeviceBuffer.from_host(enc)
        dpts, st = codec.decode_statuses(dbuf, g.gid, n_eff, raw=raw, out_device=True)
        assert (dpts.to_host(n_eff * g.pt), st) == want
        assert codec.encode_points(dpts, g.gid, raw=raw, n=n_eff) == enc
        assert codec.decode_statuses(enc, g.gid, n_eff, raw=raw, subgroup_check=False) == want


@pytest.mark.parametrize("name", ref.GROUP_NAMES)
def test_statuses_gpu_equal_host(name, chunk):
    """every malformed input between good points, 257 points in one call per encoding"""
    from gnark_amd import codec
    g = ref.group(name)
    for raw in (False, True):
        cases = [c for c in ref.bad_cases(name) if c[1] == raw]
        mont, enc = ref.encoded(name, raw, 257)
        e = g.esz(raw)
        blob = bytearray(enc)
        where = {}
        for j, c in enumerate(cases):
            i = 3 + 31 * j  # spread over waves, blocks and (chunk 128) launches
            assert i < 257
            blob[i * e:(i + 1) * e] = c[2]
            where[i] = c
        for checks in (True, False):
            want = codec.decode_statuses(bytes(blob), g.gid, 257, raw=raw, subgroup_check=checks, host=True)
            for i, c in where.items():
                expect = c[3] if checks else c[4]
                if expect is not None:
                    assert want[1][i] == expect, c[0]
            assert sum(1 for s in want[1] if s) <= len(cases)
            assert codec.decode_statuses(bytes(blob), g.gid, 257, raw=raw, subgroup_check=checks) == want
        with pytest.raises(ValueError, match="point 3: "):
            codec.decode_points(bytes(blob), g.gid, 257, raw=raw)


# ---------------------------------------------------------------- 7. the bellman vectors
def test_bellman_vectors_gpu():
    check_bellman_vectors("gpu", False)


# ---------------------------------------------------------------- 8. keys from the GPU setup
def _same_key(a, b):
    for f in ("log_n", "g1_A", "g1_B", "g1_Z", "g1_K", "alpha1", "beta1", "delta1", "g2_B", "beta2", "delta2",
              "nb_public", "curve"):
        assert getattr(a, f) == getattr(b, f), f
    assert bytes(a.infinity_A) == bytes(b.infinity_A) and bytes(a.infinity_B) == bytes(b.infinity_B)


@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
def test_setup_key_through_the_codec_then_prove(curve):
    """About 300 constraints: setup on the GPU, WriteTo, ReadFrom on the GPU, and
    the same proof from the read key as from the original for the same r, s."""
    from gnark_amd import backend, fr, groth16, pkio, solver
    mod, mont = (o.R, fr.fr_mont) if curve == "bn254" else (fr.BLS_R, fr.bls_fr_mont)
    rng = random.Random(1700)
    nbp, nbs, nint = 3, 4, 300
    cons = r1cs_solver.random_circuit(rng, nbp, nbs, nint, R=mod)
    nw = nbp + nbs + nint
    pk, vk = groth16.setup_from_terms(nbp, nw, cons, curve=curve)
    blob = pkio.write_proving_key(pk, raw=False, codec="gpu")
    assert blob == pkio.write_proving_key(pk, raw=False, codec="host")
    back, cks = pkio.read_proving_key(blob, nb_public=nbp, curve=curve, codec="gpu")
    assert cks == []
    _same_key(back, pk)
    assert pkio.write_proving_key(back, raw=False, codec="gpu") == blob
    vkb = pkio.write_verifying_key(vk, codec="gpu")
    assert pkio.read_verifying_key(vkb, curve=curve, codec="gpu") == vk
    wit = [rng.randrange(mod) for _ in range(nbp - 1 + nbs)]
    r, s = mont(0x5EED0001), mont(0x5EED0002)
    proofs = []
    for data in (pk, back):
        dev = groth16.ProvingKey(data)
        sys_ = solver.R1CS.from_terms(nbp, nbs, nw, cons, curve=curve)
        try:
            proofs.append(groth16.prove(dev, sys_.solve(wit), backend.with_amd_acceleration(), r=r, s=s))
        finally:
            sys_.close()
            dev.close()
    assert (proofs[0].Ar, proofs[0].Bs, proofs[0].Krs) == (proofs[1].Ar, proofs[1].Bs, proofs[1].Krs)
    pb = pkio.write_proof(proofs[1], curve=curve, codec="gpu")
    assert pkio.read_proof(pb, curve=curve, codec="gpu") == groth16.Proof(
        proofs[1].Ar, proofs[1].Bs, proofs[1].Krs, (), bytes(len(proofs[1].Ar)))
    key = groth16.VerifyingKey(vk) if curve == "bn254" else groth16.Bls12381VerifyingKey(vk)
    try:
        assert groth16.verify_batch([pkio.read_proof(pb, curve=curve, codec="gpu")], key, [wit[:nbp - 1]]) == [0]
    finally:
        key.close()


@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
def test_setup_key_with_a_commitment_through_the_codec(curve):
    """A key with one BSB22 commitment from the GPU setup: the Pedersen bases and
    the verifying key's commitment part survive WriteTo / ReadFrom on the GPU; on
    BN254 (where the prover takes commitments) the read key proves as the original."""
    from gnark_amd import backend, fr, groth16, pedersen, pkio
    rcs, cinfo = bo.bsb22_test_circuit(1)
    tw = groth16.ToxicWaste(987654321, 1111, 2222, 3333, 4444)
    com = [(c.commitment_index, c.private_committed, c.public_committed) for c in cinfo]
    pk, vk = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, commitments=com,
                                      toxic_waste=tw, pedersen=(424242, 77), curve=curve)
    keys = [(k.basis, k.basis_exp_sigma) for k in pk.commitment_keys]
    blob = pkio.write_proving_key(pk, raw=False, commitment_keys=keys, codec="gpu")
    back, cks = pkio.read_proving_key(blob, nb_public=rcs.nb_public, k_wire_index=pk.k_wire_index, curve=curve,
                                      codec="gpu")
    assert cks == keys
    _same_key(back, pk)
    vkb = pkio.write_verifying_key(vk, codec="gpu")
    vk2 = pkio.read_verifying_key(vkb, curve=curve, codec="gpu")
    assert vk2 == vk and vk2.commitment_key_g is not None and len(vk2.public_and_commitment_committed) == 1
    if curve != "bn254":
        return
    back.commitment_keys = [pedersen.ProvingKey(b_, s_) for b_, s_ in cks]
    rp, _ = bo.setup_bsb22(rcs, o.ToxicWaste(tw.tau, tw.alpha, tw.beta, tw.gamma, tw.delta), cinfo, sigma=424242,
                           g_scalar=77)
    w, _ = bo.bsb22_test_witness(rcs, rp, x=3, a=5, b=7, c=11)
    A, B, C = rcs.solution(w)
    sol = groth16.Solution(o.fr_vec_to_bytes(w), o.fr_vec_to_bytes(A), o.fr_vec_to_bytes(B), o.fr_vec_to_bytes(C),
                           len(w), len(A))
    proofs = []
    for data in (pk, back):
        dev = groth16.ProvingKey(data)
        try:
            hints = pedersen.Bsb22Hints(dev.commitment_keys)
            c = cinfo[0]
            hints.hint(0, [w[i] for i in c.public_committed], [w[i] for i in c.private_committed])
            proofs.append(groth16.prove(dev, sol, backend.with_amd_acceleration(), r=fr.fr_mont(101),
                                        s=fr.fr_mont(103), bsb22=hints))
        finally:
            dev.close()
    assert proofs[0] == proofs[1] and len(proofs[0].Commitments) == 1
    pb = pkio.write_proof(proofs[0], codec="gpu")
    assert pkio.read_proof(pb, codec="gpu") == groth16.Proof(
        proofs[0].Ar, proofs[0].Bs, proofs[0].Krs, tuple(proofs[0].Commitments), proofs[0].CommitmentPok)

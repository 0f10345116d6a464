"""PlonK Verify over BLS12-381 on the GPU (gg_plonk_verify_batch_bls12_381;
backend/plonk/bls12-381/verify.go:45-294) and the KZG opening check
(gg_kzg_verify_bls12_381): the device path against the host path on the oracle
prover's proof and its corruptions, proofs made by the GPU prover with 0 to 70
public inputs against the Python restatement (bls_plonk_verify_ref.py), a batch
of 67 proofs with corruptions in both blocks, and setup -> prove -> verify
inside the library."""
import dataclasses
import random

import pytest

import bls12_381_oracle as o
import bls_plonk_verify_ref as ref
import plonk_prover_oracle as po
from bls_pairing_ref import g1_off_curve, g1_outside_subgroup
from plonk_circuits import Circuit, make_key
from test_bls_plonk_verify_cpu import (I_KZG, I_OUTSIDE, corruptions, instance, kzg_cases, kzg_edge_cases, lib_key,
                                       packed)

pytestmark = pytest.mark.gpu
R = o.R
OK, MALFORMED, QUOTIENT, KZG = ref.OK, ref.MALFORMED, ref.QUOTIENT, ref.KZG
G1 = o.g1_to_bytes(o.G1_GEN)


def _prove(pk, circ, seed):
    from gnark_amd import plonk_prover as pp
    L, Rv, O, pub, cmts = circ.solve(pk, seed, commit=pk.commit_lagrange)
    return pp.prove(pk, L, Rv, O, rng=random.Random(seed + 1000), public=pub, commitments=cmts), list(pub)


def _plus_g(point: bytes) -> bytes:
    return o.g1_to_bytes(o.g1_add(o.g1_from_bytes(point), o.G1_GEN))


def test_host_and_device_agree():
    from gnark_amd import plonk_verify as pv
    _, kd, tau, pr, pub = instance(5, 2, 1)
    vk = lib_key(kd, tau)
    cases = corruptions(pr, pub)
    proofs = [packed(q) for _, q, _, _ in cases] + [packed(pr)]
    wits = [w for _, _, w, _ in cases] + [pub]
    want = [st for _, _, _, st in cases] + [OK]
    assert pv.verify_batch(proofs, vk, wits) == want
    assert pv.verify_batch(proofs, vk, wits, host=True) == want
    pv.verify(packed(pr), vk, pub)
    with pytest.raises(pv.VerifyError, match="can't verify opening proof"):
        pv.verify(proofs[I_KZG], vk, pub)
    with pytest.raises(pv.VerifyError, match="invalid proof") as e:
        pv.verify(proofs[I_OUTSIDE], vk, pub)
    assert e.value.status == MALFORMED
    vk.close()


@pytest.mark.parametrize("nb_public,n_cmt", [(0, 0), (1, 0), (32, 1), (33, 0), (70, 2)])
def test_gpu_made_proofs(nb_public, n_cmt):
    """none, one, exactly one PI slice, one over a slice, three slices with the last partial"""
    from gnark_amd import plonk_verify as pv
    circ = Circuit(8, 300 + nb_public, nb_public=nb_public, n_cmt=n_cmt, curve="bls12-381")
    tau = random.Random(nb_public).randrange(2, R)
    pk = make_key(circ, tau)
    proof, pub = _prove(pk, circ, 17)
    vk = pv.Bls12381VerifyingKey(pk.vk, G1, ref.g2_bytes(tau))
    proofs, wits = [proof], [pub]
    for pos in sorted({0, nb_public // 2, nb_public - 1} if nb_public else ()):
        bad = list(pub)
        bad[pos] = (bad[pos] + 1) % R
        proofs.append(proof)
        wits.append(bad)
    got = pv.verify_batch(proofs, vk, wits)
    assert got == [OK] + [QUOTIENT] * (len(proofs) - 1)
    if (nb_public, n_cmt) in ((33, 0), (70, 2)):
        kd, g2, op = ref.key_dict_from_lib(pk.vk), ref.g2_pair(tau), ref.oracle_proof(proof)
        assert ref.verify(kd, g2, op, wits[0]) == OK
        assert ref.verify(kd, g2, op, wits[-1]) == QUOTIENT
    vk.close()
    pk.close()


def test_batch_of_67_with_corruptions():
    """two 64-lane blocks, the second with three lanes"""
    from gnark_amd import plonk_verify as pv
    circ = Circuit(6, 41, nb_public=2, n_cmt=1, curve="bls12-381")
    tau = 0xfeedc0ffee1234567
    pk = make_key(circ, tau)
    made = [_prove(pk, circ, 100 + i) for i in range(67)]
    proofs, wits = [p for p, _ in made], [w for _, w in made]
    assert proofs[1].LRO != proofs[2].LRO and wits[1] != wits[2]
    p0 = proofs[0]
    cv = list(p0.claimed_values)
    cv[2] = (cv[2] + 1) % R
    proofs[0] = dataclasses.replace(p0, claimed_values=cv)
    proofs[63] = dataclasses.replace(proofs[63], H=[proofs[63].H[0], o.g1_to_bytes(g1_outside_subgroup()),
                                                     proofs[63].H[2]])
    proofs[64] = dataclasses.replace(proofs[64], z_shifted_H=_plus_g(proofs[64].z_shifted_H))
    wits[66] = [wits[66][0], (wits[66][1] + 1) % R]
    want = [OK] * 67
    want[0], want[63], want[64], want[66] = QUOTIENT, MALFORMED, KZG, QUOTIENT
    vk = pv.Bls12381VerifyingKey(pk.vk, G1, ref.g2_bytes(tau))
    assert pv.verify_batch(proofs, vk, wits) == want
    # the key keeps no state: the same batch again, then two proofs alone
    assert pv.verify_batch(proofs, vk, wits) == want
    assert pv.verify_batch([proofs[1]], vk, [wits[1]]) == [OK]
    assert pv.verify_batch([proofs[0]], vk, [wits[0]]) == [QUOTIENT]
    assert pv.verify_batch([proofs[63]], vk, [wits[63]]) == [MALFORMED]
    kd, g2 = ref.key_dict_from_lib(pk.vk), ref.g2_pair(tau)
    for i in (0, 1, 63, 64, 66):
        assert ref.verify(kd, g2, ref.oracle_proof(proofs[i]), wits[i]) == want[i], i
    vk.close()
    pk.close()


def test_kzg_verify_on_the_device():
    from gnark_amd import kzg
    tau = 0x1234567890abcdef1234567
    rnd = random.Random(5)
    f = [rnd.randrange(R) for _ in range(8)]
    c = o.g1_mul(o.G1_GEN, po.horner(f, tau, R))
    cases = []
    for i in range(65):
        z = rnd.randrange(R)
        y = po.horner(f, z, R)
        h = o.g1_mul(o.G1_GEN, po.horner(po._div_x_minus_a(f, y, z, R), tau, R))
        cases.append((c, h, z, (y + 1) % R if i in (0, 64) else y, i not in (0, 64)))
    cases += kzg_cases(tau)[2:]  # H at infinity, z = 0, y = 0
    cases += kzg_edge_cases(tau)  # a digest off the curve, a quotient and a digest outside the subgroup
    cases.append((c, g1_off_curve(8), cases[1][2], cases[1][3], False))
    b = o.g1_to_bytes
    args = (G1, ref.g2_bytes(tau), [b(x[0]) for x in cases], [b(x[1]) for x in cases], [x[2] for x in cases],
            [x[3] for x in cases])
    got = kzg.verify(*args, curve="bls12-381")
    assert got == [x[4] for x in cases]
    assert got == kzg.verify(*args, host=True, curve="bls12-381")


def test_setup_prove_verify_round_trip():
    """plonk_prover.setup's key proves, its VerifyingKey verifies"""
    import scs_solver as ss
    from gnark_amd import plonk_prover as pp, plonk_verify as pv, solver
    from test_gpu_plonk_setup import TAU, _srs
    rng = random.Random(61)
    nbp, nbs = 3, 3
    cons, _flags, nw = ss.random_circuit(rng, R, nbp, nbs, 40)
    wit = [rng.randrange(R) for _ in range(nbp + nbs)]
    cons = ss.fill_assertions(R, cons, wit)
    sys_ = solver.SparseR1CS.from_constraints(nbp, nbs, nw, cons, curve="bls12-381")
    log_n, _ = pp.setup_sizes(len(cons), nbp)
    kzg_g1, _ = _srs("bls12-381", log_n)
    pk, pvk = pp.setup(sys_, kzg_g1)
    _W, L, Rv, O = sys_.solve(wit)
    proof = pp.prove(pk, L, Rv, O, rng=random.Random(5), public=wit[:nbp])
    vk = pv.Bls12381VerifyingKey(pvk, kzg_g1[:96], ref.g2_bytes(TAU))
    pv.verify(proof, vk, wit[:nbp])
    with pytest.raises(pv.VerifyError) as e:
        pv.verify(proof, vk, [wit[0], wit[1], (wit[2] + 1) % R])
    assert e.value.status == QUOTIENT
    vk.close()
    pk.close()

"""Groth16 Verify over BLS12-381 on the GPU (gg_groth16_verify_batch_bls12_381)
against the host run of the same per-proof functions and against verdicts known
by construction: the reference's bellman vectors, a proof this library made on
the GPU, synthetic keys built from discrete logs (bls_groth16_ref), a batch
across the 64-lane block with one corruption of every kind, BSB22 commitments;
and the endomorphism membership checks against the multiplication by r.
Every verdict is exact."""
import random

import pytest

import bls12_381_oracle as o
import bls_groth16_ref as gr
import bls_pairing_ref as br

pytestmark = pytest.mark.gpu

CURVE = "bls12-381"
OK, SUBGROUP, PEDERSEN, PAIRING = gr.OK, gr.SUBGROUP, gr.PEDERSEN, gr.PAIRING
G1B, G2B = o.g1_to_bytes(o.G1_GEN), o.g2_to_bytes(o.G2_GEN)


def _g1_multiples(ks):
    from gnark_amd import msm
    return msm.batch_scalar_mul(msm.BLS12_381_G1, G1B, o.fr_vec_to_bytes(ks), len(ks))


def _g2_multiples(ks):
    from gnark_amd import msm
    return msm.batch_scalar_mul(msm.BLS12_381_G2, G2B, o.fr_vec_to_bytes(ks), len(ks))


def _both(proofs, vk, wits):
    """the GPU statuses, after checking that the host run gives the same"""
    from gnark_amd import groth16
    gp = [p.gproof() for p in proofs]
    got = groth16.verify_batch(gp, vk, wits)
    assert got == groth16.verify_batch(gp, vk, wits, host=True)
    return got


def test_bellman_vectors():
    cases = br.load_bellman_kats()
    want = [OK if c["ok"] else PAIRING for c in cases]
    assert want.count(OK) == 6 and want.count(PAIRING) == 6
    got = gr.kat_statuses(cases, host=False)
    assert got == want and got == gr.kat_statuses(cases, host=True)


def test_gpu_made_cubic_proof():
    """the cubic circuit (x^3 + x + 5 = y): Setup, Solve and Prove on the GPU, then Verify"""
    import bn254_oracle as bn
    from gnark_amd import backend, groth16, solver
    rcs = bn.cubic_r1cs()
    pkd, vkd = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, curve=CURVE)
    pk = groth16.ProvingKey(pkd)
    sys_ = solver.R1CS.from_terms(rcs.nb_public, rcs.nb_secret, rcs.nb_wires, rcs.constraints, curve=CURVE)
    proof = groth16.prove(pk, sys_.solve([35, 3]), backend.with_amd_acceleration())
    sys_.close()
    pk.close()
    vk = groth16.Bls12381VerifyingKey(vkd)
    assert (vk.nb_public, vk.n_commitments) == (2, 0)
    assert groth16.verify_batch([proof, proof], vk, [[35], [36]]) == [OK, PAIRING]
    assert groth16.verify_batch([proof, proof], vk, [[35], [36]], host=True) == [OK, PAIRING]
    groth16.verify(proof, vk, [35])
    with pytest.raises(groth16.VerifyError, match="pairing doesn't match") as e:
        groth16.verify(proof, vk, [36])
    assert e.value.status == PAIRING
    bad = groth16.Proof(proof.Ar, o.g2_to_bytes(br.twist_point_outside_subgroup(5)), proof.Krs)
    with pytest.raises(groth16.VerifyError, match="not in the correct subgroup"):
        groth16.verify(bad, vk, [35])
    with pytest.raises(ValueError, match="invalid witness size, got 2, expected 1"):
        groth16.verify(proof, vk, [35, 3])
    vk.close()


@pytest.mark.parametrize("nb_inputs", [0, 1, 9, 70])
def test_synthetic_instances(nb_inputs):
    """0, 1 and r - 1 among the public inputs; 9 crosses the 8-input slice, 70
    fills eight full slices and a ragged one; one flipped element fails"""
    from gnark_amd import groth16
    key = gr.SyntheticKey(nb_inputs, seed=900 + nb_inputs, g1_multiples=_g1_multiples)
    for i in {0, nb_inputs // 2, nb_inputs}:       # K itself, against the oracle
        assert key.K[i] == o.g1_mul(o.G1_GEN, key.k[i]), i
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    rng = random.Random(nb_inputs)
    special = [0, 1, o.R - 1]
    wit = [special[i % 3] if i % 4 != 3 else rng.randrange(o.R) for i in range(nb_inputs)]
    proofs, wits = [key.prove(wit)], [wit]
    if nb_inputs:
        assert {0, 1, o.R - 1} <= set(wit) or nb_inputs < 3
        alt = [rng.randrange(o.R) for _ in range(nb_inputs)]
        proofs.append(key.prove(alt))
        wits.append(alt)
        for pos in sorted({0, nb_inputs // 2, nb_inputs - 1}):      # a flipped element, first / middle / last
            bad = list(wit)
            bad[pos] = (bad[pos] + 1) % o.R
            proofs.append(proofs[0])
            wits.append(bad)
    st = groth16.verify_batch([p.gproof() for p in proofs], vk, wits)
    assert st[:2] == [OK, OK][:len(st[:2])]
    assert st[2:] == [PAIRING] * len(st[2:])
    if nb_inputs <= 9:
        assert st == groth16.verify_batch([p.gproof() for p in proofs], vk, wits, host=True)
    vk.close()


def test_unused_public_input():
    """K[2] at infinity: its table row is all infinity and adds nothing, whatever the dead input is"""
    from gnark_amd import groth16
    key, proofs, wits, want = gr.unused_input_case()
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    assert groth16.verify_batch([p.gproof() for p in proofs], vk, wits) == want == [OK, OK, OK, PAIRING]
    vk.close()


def test_batch_of_67_with_every_corruption():
    from gnark_amd import groth16
    key = gr.SyntheticKey(3, seed=67)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    rng = random.Random(4)
    wits = [[rng.randrange(o.R), i, rng.randrange(o.R)] for i in range(67)]
    proofs, (a, b, c) = key.prove_many(wits, _g1_multiples, _g2_multiples)
    for i in (0, 33, 66):                          # the proofs' points, against the oracle
        assert proofs[i].ar == o.g1_mul(o.G1_GEN, a[i]) and proofs[i].krs == o.g1_mul(o.G1_GEN, c[i]), i
        assert proofs[i].bs == o.g2_mul(o.G2_GEN, b[i]), i
    outside = br.g1_outside_subgroup()
    proofs[0] = proofs[0].replace(krs=o.g1_add(proofs[0].krs, o.G1_GEN))          # wrong Krs
    proofs[63] = proofs[63].replace(ar=br.g1_off_curve(63))                       # Ar off the curve
    proofs[64] = proofs[64].replace(bs=br.twist_point_outside_subgroup(64))       # Bs outside G2
    proofs[65] = proofs[65].replace(ar=outside)                                   # Ar on the curve, outside G1
    wits[66][1] = 67                                                              # wrong witness
    assert o.on_curve(outside)
    want = [OK] * 67
    want[0], want[63], want[64], want[65], want[66] = PAIRING, SUBGROUP, SUBGROUP, SUBGROUP, PAIRING
    gp = [p.gproof() for p in proofs]
    got = groth16.verify_batch(gp, vk, wits)
    assert got == want
    # the key keeps no state: the same batch again, and single proofs
    assert groth16.verify_batch(gp, vk, wits) == want
    for i in (1, 0, 65):
        assert groth16.verify_batch([gp[i]], vk, [wits[i]]) == [want[i]]
    assert groth16.verify_batch(gp, vk, wits, host=True) == want
    with pytest.raises(groth16.VerifyError, match="not in the correct subgroup"):
        groth16.verify(gp[64], vk, wits[64])
    vk.close()


@pytest.mark.parametrize("nc", [1, 2])
def test_bsb22_commitments(nc):
    from gnark_amd import groth16
    key = gr.SyntheticKey(2, seed=220 + nc, nc=nc)
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    assert vk.n_commitments == nc
    wit = [3, 5]
    p = key.prove(wit)
    bad_pok = p.replace(pok=o.g1_add(p.pok, o.G1_GEN))
    doubled = p.replace(commitments=[o.g1_mul(p.commitments[0], 2)] + p.commitments[1:])
    off_c = p.replace(commitments=p.commitments[:-1] + [br.g1_off_curve(8)])
    inf_c = key.prove(wit, cs=[0] * (nc - 1) + [0])           # every commitment at infinity (so the PoK too)
    inf_last = key.prove(wit, cs=[77] * (nc - 1) + [0])       # the last commitment at infinity
    assert inf_c.commitments == [o.INF] * nc and inf_c.pok is o.INF and inf_last.commitments[-1] is o.INF
    # A doubled commitment changes the folded commitment but not the PoK: PEDERSEN.
    # Input 1 is committed, so [4, 5] changes h_0: with one commitment the folded
    # commitment is C_0 whatever the hashes (the Pedersen check passes, the
    # equation fails); with two the folding challenge moves and the PoK no longer fits.
    cases = [(p, wit, OK), (bad_pok, wit, PEDERSEN), (doubled, wit, PEDERSEN),
             (p, [4, 5], PAIRING if nc == 1 else PEDERSEN), (off_c, wit, SUBGROUP), (inf_c, wit, OK),
             (inf_last, wit, OK), (p, [3, 6], PAIRING)]
    got = _both([q for q, _, _ in cases], vk, [w for _, w, _ in cases])
    assert got == [st for _, _, st in cases]
    assert _both([p], vk, [wit]) == [OK]
    assert _both([q for q, _, _ in cases], vk, [w for _, w, _ in cases]) == got
    with pytest.raises(groth16.VerifyError, match="proof of knowledge"):
        groth16.verify(bad_pok.gproof(), vk, wit)
    vk.close()


def _scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, o.R) for _ in range(n)]


def test_g1_endomorphism_check_equals_the_multiplication_by_r():
    from gnark_amd import pairing
    ks = _scalars(66, 6)
    pts = bytearray(_g1_multiples(ks))
    want = [0] * 66
    outside = br.g1_outside_subgroup()
    for i, (p, flag) in {0: (br.g1_off_curve(3), 1), 5: (None, 0), 63: (outside, 2), 64: (br.g1_off_curve(4), 1),
                         65: (outside, 2)}.items():
        pts[96 * i:96 * (i + 1)] = o.g1_to_bytes(p)
        want[i] = flag
    # a point of the cofactor's torsion (r times a point outside the subgroup), alone and added to subgroup points
    torsion = o.g1_mul_raw(outside, o.R)
    assert torsion is not o.INF and o.on_curve(torsion)
    extra = [(torsion, 2)] + [(o.g1_add(o.g1_mul(o.G1_GEN, k), torsion), 2) for k in (1, 2, 0xABCDEF)]
    extra += [(br.g1_off_curve(s), 1) for s in (5, 6, 7)] + [(o.g1_mul(o.G1_GEN, o.R - 1), 0)]
    for p, flag in extra:
        pts += o.g1_to_bytes(p)
        want.append(flag)
    assert all(want.count(f) >= 5 for f in (0, 1, 2))
    plain = pairing.g1_check(bytes(pts), curve=CURVE)
    assert plain == want
    assert pairing.g1_check(bytes(pts), curve=CURVE, endo=True) == plain


def test_g2_endomorphism_check_equals_the_multiplication_by_r():
    from gnark_amd import pairing
    ks = _scalars(66, 5)
    pts = bytearray(_g2_multiples(ks))
    want = [0] * 66
    outside = br.twist_point_outside_subgroup(3)
    for i, (q, flag) in {0: (br.g2_off_twist(9), 1), 5: (None, 0), 63: (outside, 2), 64: (br.g2_off_twist(10), 1),
                         65: (outside, 2)}.items():
        pts[192 * i:192 * (i + 1)] = o.g2_to_bytes(q)
        want[i] = flag
    extra = [(br.twist_point_outside_subgroup(s), 2) for s in (11, 12, 13)]
    extra += [(br.g2_off_twist(s), 1) for s in (11, 12, 13)] + [(o.g2_mul(o.G2_GEN, o.R - 1), 0)]
    for q, flag in extra:
        pts += o.g2_to_bytes(q)
        want.append(flag)
    assert all(want.count(f) >= 5 for f in (0, 1, 2))
    plain = pairing.g2_check(bytes(pts), curve=CURVE)
    assert plain == want
    assert pairing.g2_check(bytes(pts), curve=CURVE, endo=True) == plain


def test_endo_is_refused_over_bn254():
    from gnark_amd import pairing
    with pytest.raises(ValueError, match="bls12-381"):
        pairing.g1_check(bytes(64), endo=True)

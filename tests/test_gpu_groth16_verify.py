"""Groth16 Verify on the GPU (gg_groth16_verify_batch; verify.go:43-140) against
the oracle's verifier: the golden cubic proof, a proof made by the GPU prover,
synthetic instances with 0 to 300 public inputs, a batch with one corruption
of every kind, and BSB22 proofs with one and two commitments."""
import pytest

import bn254_oracle as o
import bn254_bsb22 as bo
import pairing_ref as pr
from helpers import b, golden

pytestmark = pytest.mark.gpu

OK, SUBGROUP, PEDERSEN, PAIRING = 0, 1, 2, 3
CUBIC_TW = (1234567, 891011, 121314, 151617, 181920)   # the golden cubic key's toxic waste


def _gproof(p):
    from gnark_amd import groth16
    return groth16.Proof(o.g1_to_bytes(p.Ar), o.g2_to_bytes(p.Bs), o.g1_to_bytes(p.Krs))


def _cubic_vk():
    from gnark_amd import groth16
    _, vk = o.setup(o.cubic_r1cs(), o.ToxicWaste(*CUBIC_TW))
    return vk, groth16.VerifyingKey(pr.vk_data_from_oracle(vk, 2))


def test_golden_cubic_proof():
    from gnark_amd import groth16
    g = golden()["groth16"][0]
    ovk, vk = _cubic_vk()
    assert o.g2_to_bytes(ovk.g2_beta).hex() == g["beta2"]      # the golden key is this setup's
    proof = groth16.Proof(b(g["Ar"]), b(g["Bs"]), b(g["Krs"]))
    oproof = o.Proof(o.g1_from_bytes(proof.Ar), o.g2_from_bytes(proof.Bs), o.g1_from_bytes(proof.Krs))
    assert groth16.verify_batch([proof, proof], vk, [[35], [36]]) == [OK, PAIRING]
    assert o.verify(oproof, ovk, [35]) and not o.verify(oproof, ovk, [36])
    groth16.verify(proof, vk, [35])
    with pytest.raises(groth16.VerifyError, match="pairing doesn't match"):
        groth16.verify(proof, vk, [36])
    with pytest.raises(ValueError, match="invalid witness size"):
        groth16.verify(proof, vk, [35, 1])
    vk.close()


def test_gpu_made_proof_verifies():
    """prove and verify inside the library: random r, s"""
    from gnark_amd import backend, groth16
    g = golden()["groth16"][0]
    pk = groth16.ProvingKey(groth16.ProvingKeyData(
        log_n=g["log_n"], g1_A=b(g["g1_A"]), g1_B=b(g["g1_B"]), g1_Z=b(g["g1_Z"]),
        g1_K=b(g["g1_K"]), alpha1=b(g["alpha1"]), beta1=b(g["beta1"]), delta1=b(g["delta1"]),
        g2_B=b(g["g2_B"]), beta2=b(g["beta2"]), delta2=b(g["delta2"]),
        infinity_A=b(g["infA"]), infinity_B=b(g["infB"]), nb_public=g["nb_public"]))
    rcs = o.cubic_r1cs()
    w = o.cubic_witness()
    A, B, C = rcs.solution(w)
    sol = groth16.Solution(o.fr_vec_to_bytes(w), o.fr_vec_to_bytes(A), o.fr_vec_to_bytes(B),
                           o.fr_vec_to_bytes(C), len(w), len(A))
    proof = groth16.prove(pk, sol, backend.with_amd_acceleration())
    _, vk = _cubic_vk()
    groth16.verify(proof, vk, [35])
    with pytest.raises(groth16.VerifyError) as e:
        groth16.verify(proof, vk, [34])
    assert e.value.status == PAIRING
    vk.close()


@pytest.mark.parametrize("nb_inputs", [0, 1, 70, 300])
def test_synthetic_instances(nb_inputs):
    """0, 1 and r - 1 among the public inputs; one flipped element fails"""
    from gnark_amd import groth16
    key = pr.SyntheticKey(nb_inputs, seed=900 + nb_inputs)
    vk = groth16.VerifyingKey(key.vk_data())
    rng = o.SplitMix64(nb_inputs)
    special = [0, 1, o.R - 1]
    wit = [special[i % 3] if i % 4 != 3 else rng.fr() for i in range(nb_inputs)]
    proofs, wits = [_gproof(key.prove(wit))], [wit]
    if nb_inputs:
        alt = [rng.fr() for _ in range(nb_inputs)]
        proofs.append(_gproof(key.prove(alt)))
        wits.append(alt)
        for pos in {0, nb_inputs - 1, nb_inputs // 2}:      # a flipped element, first / middle / last
            bad = list(wit)
            bad[pos] = (bad[pos] + 1) % o.R
            proofs.append(proofs[0])
            wits.append(bad)
    st = groth16.verify_batch(proofs, vk, wits)
    assert st[:2] == [OK, OK][:len(st[:2])]
    assert st[2:] == [PAIRING] * len(st[2:])
    if nb_inputs in (0, 1):     # the oracle agrees (its scalar multiplications are slow for many inputs)
        assert o.verify(key.prove(wit), key.vk, wit)
    vk.close()


def test_unused_public_input():
    """A public input that no constraint uses: K[2] is the infinity, its table row
    is all infinity and adds nothing, whatever the dead input is"""
    from gnark_amd import groth16
    key = pr.SyntheticKey(2, seed=77, zero_k=(2,))
    assert key.vk.g1_K[2] is None and key.vk.g1_K[1] is not None
    vk = groth16.VerifyingKey(key.vk_data())
    dead = int.from_bytes(bytes(range(0x11, 0x31)), "big")          # 32 nonzero bytes, < r
    wits = [[5, dead], [o.R - 2, o.R - 1], [5, dead ^ 0xFF00FF], [6, dead]]
    p1, p2 = key.prove(wits[0]), key.prove(wits[1])
    proofs, want = [p1, p2, p1, p1], [OK, OK, OK, PAIRING]
    assert groth16.verify_batch([_gproof(p) for p in proofs], vk, wits) == want
    for p, w, st in zip(proofs, wits, want):
        assert o.verify(p, key.vk, w) == (st == OK)
    vk.close()


def test_batch_with_every_corruption():
    from gnark_amd import groth16
    key = pr.SyntheticKey(3, seed=67)
    vk = groth16.VerifyingKey(key.vk_data())
    rng = o.SplitMix64(4)
    wits = [[rng.fr(), i, rng.fr()] for i in range(67)]
    oproofs = [key.prove(w) for w in wits]
    oproofs[0] = o.Proof(oproofs[0].Ar, oproofs[0].Bs, o.g1_add(oproofs[0].Krs, o.G1_GEN))          # wrong Krs
    oproofs[63] = o.Proof(pr.g1_off_curve(63), oproofs[63].Bs, oproofs[63].Krs)                      # Ar off the curve
    oproofs[64] = o.Proof(oproofs[64].Ar, pr.twist_point_outside_subgroup(64), oproofs[64].Krs)      # Bs outside G2
    wits[66][1] = 67                                                                                  # wrong witness
    want = [OK] * 67
    want[0], want[63], want[64], want[66] = PAIRING, SUBGROUP, SUBGROUP, PAIRING
    got = groth16.verify_batch([_gproof(p) for p in oproofs], vk, wits)
    assert got == want
    for i in (0, 63, 64, 66, 1, 62, 65):
        assert o.verify(oproofs[i], key.vk, wits[i]) == (want[i] == OK), i
    # the key keeps no state: the same batch again, and its first proof alone
    assert groth16.verify_batch([_gproof(p) for p in oproofs], vk, wits) == want
    assert groth16.verify_batch([_gproof(oproofs[1])], vk, [wits[1]]) == [OK]
    assert groth16.verify_batch([_gproof(oproofs[0])], vk, [wits[0]]) == [PAIRING]
    with pytest.raises(groth16.VerifyError, match="not in the correct subgroup"):
        groth16.verify(_gproof(oproofs[64]), vk, wits[64])
    vk.close()


@pytest.mark.parametrize("nc", [1, 2])
def test_bsb22_commitments(nc):
    from gnark_amd import groth16
    rcs, cinfo = bo.bsb22_test_circuit(nc)
    tw = o.ToxicWaste(t=987654321, alpha=1111, beta=2222, gamma=3333, delta=4444)
    pk, ovk = bo.setup_bsb22(rcs, tw, cinfo, sigma=424242, g_scalar=77)
    w, pts = bo.bsb22_test_witness(rcs, pk, x=3, a=5, b=7, c=11)
    p = bo.prove_bsb22(rcs, pk, w, pts, r=101, s=103)
    pub = w[1:rcs.nb_public]
    vk = groth16.VerifyingKey(pr.vk_data_from_oracle(ovk, rcs.nb_public, bsb22=True))
    assert vk.n_commitments == nc

    def gp(q):
        return groth16.Proof(o.g1_to_bytes(q.Ar), o.g2_to_bytes(q.Bs), o.g1_to_bytes(q.Krs),
                             [o.g1_to_bytes(c) for c in q.commitments], o.g1_to_bytes(q.pok))
    bad_pok = bo.ProofBsb22(p.Ar, p.Bs, p.Krs, p.commitments, o.g1_add(p.pok, o.G1_GEN))
    bad_c = bo.ProofBsb22(p.Ar, p.Bs, p.Krs, [o.g1_mul(p.commitments[0], 2)] + p.commitments[1:], p.pok)
    off_c = bo.ProofBsb22(p.Ar, p.Bs, p.Krs, p.commitments[:-1] + [pr.g1_off_curve(8)], p.pok)
    cases = [(p, pub), (bad_pok, pub), (bad_c, pub), (p, [4]), (off_c, pub)]
    got = groth16.verify_batch([gp(q) for q, _ in cases], vk, [x for _, x in cases])
    assert got[0] == OK and got[1] == PEDERSEN and got[4] == SUBGROUP
    assert got[2] != OK and got[3] != OK
    for (q, x), st in zip(cases[:4], got):
        assert bo.verify_bsb22(q, ovk, x) == (st == OK)
    assert groth16.verify_batch([gp(p)], vk, [pub]) == [OK]
    assert groth16.verify_batch([gp(q) for q, _ in cases], vk, [x for _, x in cases]) == got
    vk.close()

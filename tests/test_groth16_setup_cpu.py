"""Groth16 Setup, the host-only part: gg_groth16_setup_layout (the K split of
backend/groth16/bn254/setup.go:159-196) against a Python restatement of that
loop, and its refusals.  No GPU: the function must not touch the device."""
import random

import pytest

import bn254_bsb22 as bo

VK, PK, CK = 0, 1, 2


def _restated(n_wires, nb_public, commitment_wires, private_committed):
    """setup.go:159-196 line by line: (class, slot) per wire and the class sizes."""
    nc = len(commitment_wires)
    cls, slot = [None] * n_wires, [None] * n_wires
    vI, cI, seen, nb_cseen = 0, [0] * nc, 0, 0
    for i in range(n_wires):
        commitment, is_commitment = -1, False
        is_public = i < nb_public
        if not is_public:
            if nb_cseen < nc and commitment_wires[nb_cseen] == i:
                is_commitment = True
                nb_cseen += 1
            for j in range(nc):
                if cI[j] < len(private_committed[j]) and private_committed[j][cI[j]] == i:
                    commitment = j
                    break
        if is_public or commitment != -1 or is_commitment:
            if is_public or is_commitment:
                cls[i], slot[i] = VK, vI
                vI += 1
            else:
                cls[i], slot[i] = CK + commitment, cI[commitment]
                cI[commitment] += 1
                seen += 1
        else:
            cls[i], slot[i] = PK, i - vI - seen
    return cls, slot, vI, n_wires - vI - seen, cI


def _layout(n_wires, nb_public, cw, pc):
    from gnark_amd import groth16
    cls, slot, nvk, npk, nck = groth16.setup_layout(n_wires, nb_public, cw, pc)
    return list(map(int, cls)), list(map(int, slot)), nvk, npk, nck


@pytest.mark.parametrize("seed", range(12))
def test_layout_random_partitions(seed):
    rng = random.Random(1000 + seed)
    n_wires = 200 + rng.randrange(-7, 8)
    nb_public = rng.randrange(1, 20)
    nc = seed % 4  # 0 to 3 commitments
    pool = list(range(nb_public, n_wires))
    rng.shuffle(pool)
    cw = sorted(pool[:nc])
    rest = pool[nc:]
    pc, at = [], 0
    for _ in range(nc):
        m = rng.randrange(0, 25)
        pc.append(sorted(rest[at:at + m]))
        at += m
    assert _layout(n_wires, nb_public, cw, pc) == tuple(_restated(n_wires, nb_public, cw, pc))


def test_layout_bsb22_circuit():
    from gnark_amd import pedersen
    rcs, cinfo = bo.bsb22_test_circuit(2)
    cw = [c.commitment_index for c in cinfo]
    pc = [c.private_committed for c in cinfo]
    cls, slot, nvk, npk, nck = _layout(rcs.nb_wires, rcs.nb_public, cw, pc)
    assert (cls, slot, nvk, npk, nck) == tuple(_restated(rcs.nb_wires, rcs.nb_public, cw, pc))
    assert nvk == rcs.nb_public + 2 and nck == [2, 1]
    kidx = [i for i in range(rcs.nb_wires) if cls[i] == PK]
    assert [slot[i] for i in kidx] == list(range(npk))
    assert kidx == pedersen.k_wire_index(rcs.nb_public, rcs.nb_wires, pc, cw)


def test_layout_no_commitments():
    cls, slot, nvk, npk, nck = _layout(9, 3, [], [])
    assert cls == [VK] * 3 + [PK] * 6 and slot == [0, 1, 2, 0, 1, 2, 3, 4, 5]
    assert (nvk, npk, nck) == (3, 6, [])


@pytest.mark.parametrize("cw,pc,wire", [
    ([7, 7], [[], []], 7),            # commitment wires not strictly increasing
    ([9, 8], [[], []], 8),
    ([8], [[5, 5]], 5),               # a committed list not strictly increasing
    ([8], [[6, 4]], 4),
    ([8], [[2]], 2),                  # a committed wire below nb_public
    ([1], [[]], 1),                   # a commitment wire below nb_public
    ([8], [[12]], 12),                # at n_wires
    ([13], [[]], 13),                 # above n_wires
    ([8, 9], [[5], [4, 5]], 5),       # a wire in two commitments
    ([8, 9], [[4], [8]], 8),          # a commitment wire privately committed
])
def test_layout_refusals(cw, pc, wire):
    import gnark_amd
    from gnark_amd import groth16
    with pytest.raises(gnark_amd.GnarkAmdError) as e:
        groth16.setup_layout(12, 3, cw, pc)
    assert e.value.code == 1  # GG_ERR_INVALID_ARG
    assert f"wire {wire} " in str(e.value) or str(e.value).endswith(f"wire {wire}"), str(e.value)


def test_generators_match_the_oracles():
    import bn254_oracle as o
    import bls12_381_oracle as bls
    from gnark_amd import fr
    assert fr.generators("bn254") == (o.g1_to_bytes(o.G1_GEN), o.g2_to_bytes(o.G2_GEN))
    assert fr.generators("bls12-381") == (bls.g1_to_bytes(bls.G1_GEN), bls.g2_to_bytes(bls.G2_GEN))

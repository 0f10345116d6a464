"""The BN254 pairing kernels (gg_pairing_bn254, gg_pairing_check_bn254) and the
membership checks (gg_g1_check_bn254, gg_g2_check_bn254) on the GPU against
the host run of the same templates and against the oracle's pairing.  For
many products the inputs are (a_i G1, b_i G2), so the expected value is a
power of e(G1, G2) and costs no oracle pairing."""
import numpy as np
import pytest

import bn254_oracle as o
import coracle
import pairing_ref as pr

pytestmark = pytest.mark.gpu

_EM_SQUARES = []


def _e_pow(k):
    """bytes of e(G1, G2)^(k m) from cached squarings of e(G1, G2)^m"""
    from gnark_amd import pairing
    if not _EM_SQUARES:
        x = pr.e_gen() ** pairing.GT_MULTIPLE
        for _ in range(254):
            _EM_SQUARES.append(x)
            x = x * x
    k %= o.R
    acc, i = o.Fp12.one(), 0
    while k:
        if k & 1:
            acc = acc * _EM_SQUARES[i]
        k >>= 1
        i += 1
    return pr.gt_to_bytes(acc)


def _scalars(n, seed):
    rng = o.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


def _g1_multiples(ks):
    pts = coracle.g1_batch_mul(o.g1_to_bytes(o.G1_GEN), o.fr_vec_to_bytes(ks), len(ks))
    return bytes(pts)


def _g2_multiples(ks):
    pts = coracle.g2_batch_mul(o.g2_to_bytes(o.G2_GEN), o.fr_vec_to_bytes(ks), len(ks))
    return bytes(pts)


def test_gpu_host_oracle_agree_on_one_pairing():
    from gnark_amd import pairing
    p, q = o.g1_mul(o.G1_GEN, 0x1234567), o.g2_mul(o.G2_GEN, 0x7654321)
    g1, g2 = o.g1_to_bytes(p), o.g2_to_bytes(q)
    gpu = pairing.pair(g1, g2)
    assert gpu == pairing.pair(g1, g2, host=True)
    assert gpu == [pr.gt_to_bytes(o.pairing(p, q) ** pairing.GT_MULTIPLE)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_products_of_generator_multiples(n):
    """k = 1, then k = 3 with an infinity in one pair of a few products"""
    from gnark_amd import pairing
    a, b = _scalars(3 * n, 100 + n), _scalars(3 * n, 200 + n)
    g1, g2 = bytearray(_g1_multiples(a)), bytearray(_g2_multiples(b))
    got = pairing.pair(bytes(g1[:64 * n]), bytes(g2[:128 * n]), k=1)
    for i in range(n):
        assert got[i] == _e_pow(a[i] * b[i]), (n, i)
    live = [[True] * 3 for _ in range(n)]
    for i in {0, n // 2, n - 1}:          # product i: pair i % 3 has an infinity, G1 or G2 side
        j = i % 3
        live[i][j] = False
        if i & 1:
            g1[64 * (3 * i + j):64 * (3 * i + j + 1)] = bytes(64)
        else:
            g2[128 * (3 * i + j):128 * (3 * i + j + 1)] = bytes(128)
    got = pairing.pair(bytes(g1), bytes(g2), k=3)
    assert len(got) == n
    for i in range(n):
        e = sum(a[3 * i + j] * b[3 * i + j] for j in range(3) if live[i][j])
        assert got[i] == _e_pow(e), (n, i)


def test_bilinearity_on_random_points():
    """e(P, Q + Q') = e(P, Q) e(P, Q'), the right side multiplied in the oracle"""
    from gnark_amd import pairing
    rng = o.SplitMix64(77)
    p = o.g1_mul(o.G1_GEN, rng.fr())
    q, q2 = o.g2_mul(o.G2_GEN, rng.fr()), o.g2_mul(o.G2_GEN, rng.fr())
    g1 = o.g1_to_bytes(p) * 3
    g2 = o.g2_to_bytes(o.g2_add(q, q2)) + o.g2_to_bytes(q) + o.g2_to_bytes(q2)
    lhs, e1, e2 = pairing.pair(g1, g2)
    assert pr.gt_from_bytes(lhs) == pr.gt_from_bytes(e1) * pr.gt_from_bytes(e2)
    assert lhs != pr.gt_one() and e1 != e2


def test_pairing_check():
    from gnark_amd import pairing
    p, q = o.g1_mul(o.G1_GEN, 31337), o.g2_mul(o.G2_GEN, 271828)
    neg = (p[0], (-p[1]) % o.P)
    g1 = o.g1_to_bytes(p) + o.g1_to_bytes(neg) + o.g1_to_bytes(p) + o.g1_to_bytes(p)
    g2 = o.g2_to_bytes(q) * 4
    assert pairing.pairing_check(g1, g2, k=2) == [True, False]
    assert pairing.pairing_check(bytes(64) * 2, g2[:256], k=2) == [True]


def test_g2_check_mixed_points():
    from gnark_amd import pairing
    ks = _scalars(66, 5)
    pts = bytearray(_g2_multiples(ks))
    want = [0] * 66
    outside = pr.twist_point_outside_subgroup(3)
    assert pr.g2_on_twist(outside) and pr.g2_times_r(outside) is not None
    assert pr.g2_times_r(o.g2_mul(o.G2_GEN, ks[1])) is None
    for i, (q, flag) in {0: (None, 0), 7: (pr.g2_off_twist(9), 1), 63: (outside, 2), 64: (pr.g2_off_twist(10), 1),
                         65: (outside, 2), 33: (None, 0)}.items():
        pts[128 * i:128 * (i + 1)] = o.g2_to_bytes(q)
        want[i] = flag
    assert pairing.g2_check(bytes(pts)) == want


def test_g1_check_mixed_points():
    from gnark_amd import pairing
    ks = _scalars(66, 6)
    pts = bytearray(_g1_multiples(ks))
    want = [0] * 66
    for i, p in {0: pr.g1_off_curve(3), 5: None, 63: pr.g1_off_curve(4), 64: None, 65: pr.g1_off_curve(5)}.items():
        pts[64 * i:64 * (i + 1)] = o.g1_to_bytes(p)
        want[i] = 0 if p is None else 1
    assert pairing.g1_check(bytes(pts)) == want

"""BN254 optimal ate pairing and the point membership checks of Groth16 Verify
(curve.Pair / PairingCheck / IsInSubGroup as used by
backend/groth16/bn254/verify.go:61-135).

A GT value is 384 bytes in gnark-crypto's E12 memory layout.  Every value is
e(P, Q) ** GT_MULTIPLE: the final exponentiation's hard part computes a fixed
multiple of the canonical exponent (coprime to r), so products, equality and
the check "= 1" behave as for the reduced pairing."""
from __future__ import annotations

from ._lib import GG_GT_BYTES, check, lib, ptr

_X = 4965661367192848881
# m = 2x(6x^2 + 3x + 1): the pairing computed is e(P, Q)^m
GT_MULTIPLE = 2 * _X * (6 * _X * _X + 3 * _X + 1)
GT_BYTES = GG_GT_BYTES


def _count(buf, size, what):
    if len(buf) % size:
        raise ValueError(f"{what}: {len(buf)} bytes is not a multiple of {size}")
    return len(buf) // size


def _pairs(g1: bytes, g2: bytes, k: int) -> int:
    n1, n2 = _count(g1, 64, "g1"), _count(g2, 128, "g2")
    if n1 != n2 or k <= 0 or n1 % k:
        raise ValueError(f"{n1} G1 points, {n2} G2 points, k = {k}")
    return n1 // k


def pair(g1: bytes, g2: bytes, k: int = 1, host: bool = False) -> list:
    """n products of k pairs each: out[i] = prod_j e(g1[i k + j], g2[i k + j]),
    as a list of n 384-byte GT values.  host=True runs the same code on the CPU."""
    n = _pairs(g1, g2, k)
    out = bytearray(n * GT_BYTES)
    fn = lib.gg_pairing_bn254_host if host else lib.gg_pairing_bn254
    check(fn(n, k, ptr(g1), ptr(g2), ptr(out)))
    return [bytes(out[i * GT_BYTES:(i + 1) * GT_BYTES]) for i in range(n)]


def pairing_check(g1: bytes, g2: bytes, k: int) -> list:
    """One bool per product of k pairs: is it 1?"""
    n = _pairs(g1, g2, k)
    ok = bytearray(n)
    check(lib.gg_pairing_check_bn254(n, k, ptr(g1), ptr(g2), ptr(ok)))
    return [bool(x) for x in ok]


def g1_check(points: bytes) -> list:
    """One flag per G1Affine: 0 good, 1 not on the curve (cofactor 1: never 2)."""
    n = _count(points, 64, "g1")
    f = bytearray(n)
    check(lib.gg_g1_check_bn254(n, ptr(points), ptr(f)))
    return list(f)


def g2_check(points: bytes) -> list:
    """One flag per G2Affine: 0 good, 1 not on the twist, 2 not in the r-torsion."""
    n = _count(points, 128, "g2")
    f = bytearray(n)
    check(lib.gg_g2_check_bn254(n, ptr(points), ptr(f)))
    return list(f)


def hash_to_field(msg: bytes, dst: bytes = b"bsb22-commitment") -> bytes:
    """fr.Hash(msg, dst, 1): one fr in Montgomery form (32 bytes)."""
    out = bytearray(32)
    check(lib.gg_hash_to_field_bn254(ptr(msg) if msg else None, len(msg), ptr(dst) if dst else None, len(dst),
                                     ptr(out)))
    return bytes(out)

"""Optimal ate pairings and the point membership checks of the verifiers
(curve.Pair / PairingCheck / IsInSubGroup as used by
backend/groth16/bn254/verify.go:61-135), over BN254 (the default) and, with
curve="bls12-381", over BLS12-381.

A GT value is gnark-crypto's E12 memory layout: 384 bytes over BN254, 576 bytes
over BLS12-381.  Every value is e(P, Q) ** GT_MULTIPLE (BN254) or
e(P, Q) ** GT_MULTIPLE_BLS12_381 (BLS12-381): the final exponentiation's hard
part computes a fixed multiple of the canonical exponent (coprime to r), so
products, equality and the check "= 1" behave as for the reduced pairing."""
from __future__ import annotations

from ._lib import GG_GT_BYTES, GG_GT_BYTES_BLS12_381, check, lib, ptr

_X = 4965661367192848881
# m = 2x(6x^2 + 3x + 1): the pairing computed is e(P, Q)^m
GT_MULTIPLE = 2 * _X * (6 * _X * _X + 3 * _X + 1)
GT_BYTES = GG_GT_BYTES
# BLS12-381: 3 Phi_12(p) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3, so e(P, Q)^3
GT_MULTIPLE_BLS12_381 = 3
GT_BYTES_BLS12_381 = GG_GT_BYTES_BLS12_381


class _Curve:
    def __init__(self, g1, g2, gt, suffix):
        self.g1, self.g2, self.gt = g1, g2, gt
        self.pair = getattr(lib, "gg_pairing_" + suffix)
        self.pair_host = getattr(lib, "gg_pairing_" + suffix + "_host")
        self.pairing_check = getattr(lib, "gg_pairing_check_" + suffix)
        self.g1_check = getattr(lib, "gg_g1_check_" + suffix)
        self.g2_check = getattr(lib, "gg_g2_check_" + suffix)
        # the endomorphism checks exist where G1 has a cofactor (BLS12-381)
        self.g1_check_endo = getattr(lib, "gg_g1_check_endo_" + suffix, None)
        self.g2_check_endo = getattr(lib, "gg_g2_check_endo_" + suffix, None)
        self.hash_to_field = getattr(lib, "gg_hash_to_field_" + suffix)


_CURVES = {}


def _curve(name: str) -> _Curve:
    if name not in ("bn254", "bls12-381"):
        raise ValueError(f"unknown curve {name!r}: the pairing runs over 'bn254' and 'bls12-381'")
    if name not in _CURVES:
        _CURVES[name] = (_Curve(64, 128, GT_BYTES, "bn254") if name == "bn254"
                         else _Curve(96, 192, GT_BYTES_BLS12_381, "bls12_381"))
    return _CURVES[name]


def _count(buf, size, what):
    if len(buf) % size:
        raise ValueError(f"{what}: {len(buf)} bytes is not a multiple of {size}")
    return len(buf) // size


def _pairs(c: _Curve, g1: bytes, g2: bytes, k: int) -> int:
    n1, n2 = _count(g1, c.g1, "g1"), _count(g2, c.g2, "g2")
    if n1 != n2 or k <= 0 or n1 % k:
        raise ValueError(f"{n1} G1 points, {n2} G2 points, k = {k}")
    return n1 // k


def pair(g1: bytes, g2: bytes, k: int = 1, host: bool = False, curve: str = "bn254") -> list:
    """n products of k pairs each: out[i] = prod_j e(g1[i k + j], g2[i k + j]),
    as a list of n GT values (384 bytes, 576 over BLS12-381).  host=True runs the
    same code on the CPU."""
    c = _curve(curve)
    n = _pairs(c, g1, g2, k)
    out = bytearray(n * c.gt)
    fn = c.pair_host if host else c.pair
    check(fn(n, k, ptr(g1), ptr(g2), ptr(out)))
    return [bytes(out[i * c.gt:(i + 1) * c.gt]) for i in range(n)]


def pairing_check(g1: bytes, g2: bytes, k: int, curve: str = "bn254") -> list:
    """One bool per product of k pairs: is it 1?"""
    c = _curve(curve)
    n = _pairs(c, g1, g2, k)
    ok = bytearray(n)
    check(c.pairing_check(n, k, ptr(g1), ptr(g2), ptr(ok)))
    return [bool(x) for x in ok]


def _check_fn(c: _Curve, which: str, endo: bool, curve: str):
    if not endo:
        return getattr(c, which)
    fn = getattr(c, which + "_endo")
    if fn is None:
        raise ValueError(f"endo=True: the endomorphism checks exist over 'bls12-381' only, not over {curve!r}")
    return fn


def g1_check(points: bytes, curve: str = "bn254", endo: bool = False) -> list:
    """One flag per G1Affine: 0 good, 1 not on the curve, 2 not in the subgroup
    of order r (BN254 has cofactor 1: never 2 there).  endo=True (BLS12-381):
    the same flags by [x^2] phi(P) + P = 0 instead of the multiplication by r."""
    c = _curve(curve)
    n = _count(points, c.g1, "g1")
    f = bytearray(n)
    check(_check_fn(c, "g1_check", endo, curve)(n, ptr(points), ptr(f)))
    return list(f)


def g2_check(points: bytes, curve: str = "bn254", endo: bool = False) -> list:
    """One flag per G2Affine: 0 good, 1 not on the twist, 2 not in the r-torsion.
    endo=True (BLS12-381): the same flags by psi(Q) = [x] Q."""
    c = _curve(curve)
    n = _count(points, c.g2, "g2")
    f = bytearray(n)
    check(_check_fn(c, "g2_check", endo, curve)(n, ptr(points), ptr(f)))
    return list(f)


def hash_to_field(msg: bytes, dst: bytes = b"bsb22-commitment", curve: str = "bn254") -> bytes:
    """fr.Hash(msg, dst, 1): one fr of the curve's scalar field in Montgomery form (32 bytes)."""
    out = bytearray(32)
    check(_curve(curve).hash_to_field(ptr(msg) if msg else None, len(msg), ptr(dst) if dst else None, len(dst),
                                      ptr(out)))
    return bytes(out)

"""KZG helpers: the Lagrange form of a canonical SRS on the GPU
(kzg.ToLagrangeG1, backend/plonk/bls12-381/setup.go:134) over the C ABI's
gg_kzg_to_lagrange_g1 (csrc/ecntt.hip: an inverse DFT over G1 points), the same
over G2 (gg_kzg_to_lagrange_g2, csrc/ecntt_g2.hip: lagrangeCoeffsG2 of
backend/groth16/bn254/mpcsetup/lagrange.go), and
kzg.Verify for batches of openings over BN254 (gg_kzg_verify_bn254,
csrc/plonk_verify.hip) or BLS12-381 (gg_kzg_verify_bls12_381,
csrc/plonk_verify_bls.hip)."""
from __future__ import annotations

from . import fr
from ._lib import DeviceBuffer, GG_CURVE_BLS12_381, GG_CURVE_BN254, check, lib, ptr


def _curve(curve: str):
    if curve == "bls12-381":
        return GG_CURVE_BLS12_381, 96, fr.bls_fr_mont, fr.bls_domain_generator
    if curve == "bn254":
        return GG_CURVE_BN254, 64, fr.fr_mont, fr.domain_generator
    raise ValueError("curve must be 'bls12-381' or 'bn254'")


def _to_lagrange(fn, scale: int, points, log_n, curve, out_device, omega, out):
    """to_lagrange_g1 / _g2: `scale` G1 point sizes per point."""
    cid, pt, mont, gen = _curve(curve)
    if not 1 <= log_n <= 27:
        raise ValueError("log_n must be in 1 .. 27")
    w = mont(omega if omega is not None else gen(log_n))
    pt *= scale
    nbytes = pt << log_n
    in_dev = isinstance(points, DeviceBuffer)
    if not in_dev:
        points = bytes(points)
        if len(points) < nbytes:
            raise ValueError("need %d points of %d bytes" % (1 << log_n, pt))
    if out is not None:
        dst, out_device = out, True
    else:
        dst = DeviceBuffer(nbytes) if out_device else bytearray(nbytes)
    check(fn(cid, log_n, ptr(w), ptr(points), int(in_dev), ptr(dst), int(out_device), None))
    return dst if out_device else bytes(dst)


def to_lagrange_g1(points, log_n: int, curve: str = "bls12-381", out_device: bool = False, omega: int = None,
                   out=None):
    """[L_i(tau)]G, i < n = 2^log_n, from points = [tau^j]G, j < n (affine, the
    curve's layout; bytes or a DeviceBuffer).  out[i] = (1/n) sum_j omega^(-ij)
    points[j] for any input points.  Returns bytes, or a DeviceBuffer with
    out_device; `out` (a DeviceBuffer, possibly `points` itself) receives the
    result in place of a new buffer.  omega: the domain's generator (default
    gnark-crypto's fft.NewDomain choice)."""
    return _to_lagrange(lib.gg_kzg_to_lagrange_g1, 1, points, log_n, curve, out_device, omega, out)


def to_lagrange_g2(points, log_n: int, curve: str = "bls12-381", out_device: bool = False, omega: int = None,
                   out=None):
    """to_lagrange_g1 over G2 points (128 B on bn254, 192 B on bls12-381):
    [tau^j]2 -> [L_i(tau)]2, the pk.G2.B side of mpcsetup.init_phase2."""
    return _to_lagrange(lib.gg_kzg_to_lagrange_g2, 2, points, log_n, curve, out_device, omega, out)


def verify(kzg_g1: bytes, kzg_g2: bytes, digests, quotients, points, values, host: bool = False,
           curve: str = "bn254") -> list:
    """kzg.Verify of n independent openings under one SRS: one bool per opening,
    e(C - y G + z H, G2) e(-H, [tau]G2) == 1.  kzg_g1: the SRS's G1 generator
    (one affine point: 64 B over BN254, 96 B over BLS12-381); kzg_g2: G2 and
    [tau]G2 (2 x 128 B, 2 x 192 B); digests C and quotients H: lists of affine
    points (all zero: the infinity); points z and values y: integers.  Over
    BLS12-381 a digest or quotient outside the order-r subgroup gives False.
    host=True runs the same code on the CPU."""
    cid, pt, mont, _ = _curve(curve)
    bls = cid == GG_CURVE_BLS12_381
    r = fr.BLS_R if bls else fr.R
    n = len(digests)
    if not (n == len(quotients) == len(points) == len(values)):
        raise ValueError("digests, quotients, points and values must have one length")
    if len(kzg_g1) < pt or len(kzg_g2) != 4 * pt:
        raise ValueError(f"kzg_g1: one G1Affine ({pt} bytes); kzg_g2: G2 and [tau]G2 ({4 * pt} bytes)")
    c, h = b"".join(bytes(x) for x in digests), b"".join(bytes(x) for x in quotients)
    if len(c) != pt * n or len(h) != pt * n:
        raise ValueError(f"a digest or a quotient is not a {pt}-byte affine point")
    z = b"".join(mont(int(x) % r) for x in points)
    y = b"".join(mont(int(x) % r) for x in values)
    ok = bytearray(n)
    if bls:
        fn = lib.gg_kzg_verify_bls12_381_host if host else lib.gg_kzg_verify_bls12_381
    else:
        fn = lib.gg_kzg_verify_bn254_host if host else lib.gg_kzg_verify_bn254
    check(fn(n, ptr(bytes(kzg_g1[:pt])), ptr(bytes(kzg_g2)), ptr(c), ptr(h), ptr(z), ptr(y), ptr(ok)))
    return [bool(x) for x in ok]

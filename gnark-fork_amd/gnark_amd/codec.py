"""gnark-crypto's point Decoder / Encoder on the GPU (gg_points_decode /
gg_points_encode, csrc/point_codec_impl.cuh): batches of G1 or G2 points of
BN254 or BLS12-381 between gnark's byte encoding (compressed or raw) and the
library's affine Montgomery layout.  host=True runs the same per-point code on
the calling thread (the `_host` entry points), with no device call.
"""
from __future__ import annotations

from ._lib import (GG_BLS12_381_G1, GG_BLS12_381_G2, GG_CURVE_BLS12_381, GG_CURVE_BN254, GG_DEC_NO_SUBGROUP_CHECK,
                   GG_ENC_COMPRESSED, GG_ENC_RAW, GG_G1, GG_G2, DeviceBuffer, check, lib, ptr)

POINT_OK, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP, POINT_BAD_ENCODING = 0, 1, 2, 3
STATUS_NAMES = {POINT_NOT_ON_CURVE: "not on the curve", POINT_NOT_IN_SUBGROUP: "not in the subgroup of order r",
                POINT_BAD_ENCODING: "bad encoding"}
# affine Montgomery bytes per point
POINT_BYTES = {GG_G1: 64, GG_G2: 128, GG_BLS12_381_G1: 96, GG_BLS12_381_G2: 192}
GROUPS = {("bn254", 1): GG_G1, ("bn254", 2): GG_G2, ("bls12-381", 1): GG_BLS12_381_G1,
          ("bls12-381", 2): GG_BLS12_381_G2}


def encoded_size(group: int, raw: bool = False) -> int:
    n = lib.gg_point_encoded_size(group, GG_ENC_RAW if raw else GG_ENC_COMPRESSED)
    if not n:
        raise ValueError(f"unknown group {group}")
    return n


def _on_device(obj) -> bool:
    return isinstance(obj, DeviceBuffer) or bool(getattr(obj, "is_cuda", False))


def decode_statuses(buf, group: int, n: int, raw: bool = False, subgroup_check: bool = True, host: bool = False,
                    out_device: bool = False):
    """(points, statuses) of n encoded points at the start of buf (bytes, numpy,
    a DeviceBuffer or a device tensor): the POINT_* status of every point, a
    point that is not OK as the infinity.  points: bytes, or a DeviceBuffer with
    out_device=True."""
    esz, psz = encoded_size(group, raw), POINT_BYTES[group]
    if n == 0:
        return (DeviceBuffer(16) if out_device else b""), b""
    in_dev = _on_device(buf)
    if not in_dev:
        if isinstance(buf, memoryview):
            buf = bytes(buf[:n * esz])
        if len(buf) < n * esz:
            raise ValueError(f"{n} points of {esz} bytes need {n * esz} bytes, got {len(buf)}")
    if host and (in_dev or out_device):
        raise ValueError("host=True takes and returns host memory")
    enc = GG_ENC_RAW if raw else GG_ENC_COMPRESSED
    flags = 0 if subgroup_check else GG_DEC_NO_SUBGROUP_CHECK
    status = bytearray(n)
    out = DeviceBuffer(n * psz) if out_device else bytearray(n * psz)
    if host:
        check(lib.gg_points_decode_host(group, enc, flags, n, ptr(buf), ptr(out), ptr(status)))
    else:
        check(lib.gg_points_decode(group, enc, flags, n, ptr(buf), int(in_dev), ptr(out), int(out_device),
                                   ptr(status)))
    return (out if out_device else bytes(out)), bytes(status)


def decode_points(buf, group: int, n: int, raw: bool = False, subgroup_check: bool = True, host: bool = False,
                  out_device: bool = False):
    """curve.Decoder over n points: the affine Montgomery points (bytes, or a
    DeviceBuffer with out_device=True).  subgroup_check=False is
    curve.NoSubgroupChecks().  Raises ValueError naming the first bad index and
    its status."""
    out, status = decode_statuses(buf, group, n, raw, subgroup_check, host, out_device)
    for i, s in enumerate(status):
        if s:
            raise ValueError(f"point {i}: {STATUS_NAMES.get(s, 'status')} (status {s})")
    return out


def encode_points(points, group: int, raw: bool = False, host: bool = False, n: int = None) -> bytes:
    """curve.Encoder (raw: RawEncoding) over affine Montgomery points (bytes,
    numpy, a DeviceBuffer or a device tensor; n is required for a tensor)."""
    esz, psz = encoded_size(group, raw), POINT_BYTES[group]
    dev = _on_device(points)
    if n is None:
        nbytes = points.nbytes if hasattr(points, "nbytes") else len(points)
        if nbytes % psz:
            raise ValueError(f"{nbytes} bytes are no whole number of {psz}-byte points")
        n = nbytes // psz
    if n == 0:
        return b""
    if host and dev:
        raise ValueError("host=True takes host memory")
    enc = GG_ENC_RAW if raw else GG_ENC_COMPRESSED
    out = bytearray(n * esz)
    if host:
        check(lib.gg_points_encode_host(group, enc, n, ptr(points), ptr(out)))
    else:
        check(lib.gg_points_encode(group, enc, n, ptr(points), int(dev), ptr(out)))
    return bytes(out)


def fp_sqrt(values, curve: str = "bn254", degree: int = 1, host: bool = False):
    """(roots, ok) of Fp (degree 1) or Fp2 (degree 2) Montgomery elements given
    as bytes: the root exactly as the decoder computes it; ok[i] = 1 iff its
    square is the input."""
    fb = (32 if curve == "bn254" else 48) * degree
    if degree not in (1, 2) or len(values) % fb:
        raise ValueError(f"values must be whole {fb}-byte elements, degree 1 or 2")
    n = len(values) // fb
    out, ok = bytearray(n * fb), bytearray(n)
    fn = lib.gg_fp_sqrt_host if host else lib.gg_fp_sqrt
    check(fn(GG_CURVE_BN254 if curve == "bn254" else GG_CURVE_BLS12_381, degree, n, ptr(values), ptr(out), ptr(ok)))
    return bytes(out), bytes(ok)

"""The point codec on the GPU: points per second, per group.

    python tools/bench_pkio.py [--log-n 20] [--reps 3] [--commit ID] [--out profiles/r17_point_codec.md]

For each of the four groups (BN254 G1 / G2, BLS12-381 G1 / G2), on 2^log_n
distinct points (random multiples of the generator from msm.batch_scalar_mul),
with the bytes and the points resident in HBM (the statuses and the encoder's
bytes come back to the host), min of --reps calls after one warm-up:

  decode     gg_points_decode, compressed, with the subgroup checks
  unsafe     the same with GG_DEC_NO_SUBGROUP_CHECK
  encode     gg_points_encode, compressed
  member     the existing membership-check kernel of the group on the same
             points in the same run (gg_g1_check_bn254, gg_g2_check_bn254,
             gg_g1_check_endo_bls12_381, gg_g2_check_endo_bls12_381)

and, on the CPU, the rate of the Python decoder (pkio.read_proving_key with
codec="python", what reading a key cost before the library codec) on a
compressed BN254 key of 2^12 G1 points.  Every decode is checked: all statuses
OK and the points equal to the input.  No threshold: the figures go to --out."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnark-fork_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _scalars(n, seed):
    s = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F  # below both group orders: a Montgomery representative of some scalar
    return s.tobytes()


def _best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def bench_group(name, n, reps):
    from gnark_amd import _lib, codec, fr, msm
    from gnark_amd._lib import check, lib, ptr
    curve, g = name.rsplit("-g", 1)
    g = int(g)
    gid = codec.GROUPS[(curve, g)]
    base = fr.generators(curve)[g - 1]
    pts = msm.batch_scalar_mul(gid, base, _scalars(n, gid), n)
    psz, esz = codec.POINT_BYTES[gid], codec.encoded_size(gid)
    dpts = _lib.DeviceBuffer.from_host(pts)
    enc = codec.encode_points(dpts, gid, n=n)
    assert len(enc) == n * esz
    denc, dout = _lib.DeviceBuffer.from_host(enc), _lib.DeviceBuffer(n * psz)
    status, out_bytes = bytearray(n), bytearray(n * esz)

    def decode(flags):
        check(lib.gg_points_decode(gid, _lib.GG_ENC_COMPRESSED, flags, n, ptr(denc), 1, ptr(dout), 1, ptr(status)))
        assert not any(status), "a valid point was refused"

    row = {"group": name}
    row["decode"] = n / _best(lambda: decode(0), reps)
    assert dout.to_host() == pts, "decoded points differ"
    row["unsafe"] = n / _best(lambda: decode(_lib.GG_DEC_NO_SUBGROUP_CHECK), reps)
    assert dout.to_host() == pts, "decoded points differ (unsafe)"
    row["encode"] = n / _best(
        lambda: check(lib.gg_points_encode(gid, _lib.GG_ENC_COMPRESSED, n, ptr(dpts), 1, ptr(out_bytes))), reps)
    assert bytes(out_bytes) == enc
    member = {"bn254-g1": lib.gg_g1_check_bn254, "bn254-g2": lib.gg_g2_check_bn254,
              "bls12-381-g1": lib.gg_g1_check_endo_bls12_381, "bls12-381-g2": lib.gg_g2_check_endo_bls12_381}[name]

    def check_members():
        check(member(n, ptr(dpts), ptr(status)))
        assert not any(status)

    row["member"] = n / _best(check_members, reps)
    return row


def bench_python_reader(n=1 << 12):
    """points/s of the Python decoder on a compressed BN254 key of n G1 points"""
    from gnark_amd import codec, fr, groth16, msm, pkio
    g1, g2 = fr.generators("bn254")
    pts = msm.batch_scalar_mul(codec.GROUPS[("bn254", 1)], g1, _scalars(n, 99), n)
    data = groth16.ProvingKeyData(
        log_n=12, g1_A=pts, g1_B=b"", g1_Z=b"", g1_K=b"", alpha1=g1, beta1=g1, delta1=g1, g2_B=b"", beta2=g2,
        delta2=g2, infinity_A=bytes(n), infinity_B=bytes([1]) * n, nb_public=1)
    blob = pkio.write_proving_key(data, raw=False, codec="host")
    t0 = time.perf_counter()
    back, _ = pkio.read_proving_key(blob, nb_public=1)
    dt = time.perf_counter() - t0
    assert back.g1_A == pts
    t0 = time.perf_counter()
    back, _ = pkio.read_proving_key(blob, nb_public=1, codec="gpu")
    dt_gpu = time.perf_counter() - t0
    assert back.g1_A == pts
    return (n + 5) / dt, (n + 5) / dt_gpu


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    box = torch.cuda.get_device_name(0)
    n = 1 << a.log_n
    rows = [bench_group(name, n, a.reps) for name in ("bn254-g1", "bn254-g2", "bls12-381-g1", "bls12-381-g2")]
    py, py_gpu = bench_python_reader()
    lines = ["# Point codec: points per second", "",
             f"Box: {box}.  Commit: {a.commit or _commit()}.  `python tools/bench_pkio.py --log-n {a.log_n} "
             f"--reps {a.reps}`.", "",
             f"2^{a.log_n} distinct points per group, compressed encoding, bytes and points in HBM, statuses (and the "
             "encoder's bytes) copied to the host; min of the timed calls after one warm-up, host wall clock "
             "around the call.  `member` is the group's existing membership-check kernel on the same points.", "",
             "| group | decode, checked | decode, unsafe | encode | member |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append("| {group} | {decode:.3e} | {unsafe:.3e} | {encode:.3e} | {member:.3e} |".format(**r))
    lines += ["", f"`pkio.read_proving_key` on a compressed BN254 key of 2^12 G1 points: codec=\"python\" "
              f"{py:.3e} points/s; codec=\"gpu\" {py_gpu:.3e} points/s (one call, launch and copies included).", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

"""PlonK Setup on the GPU: the EC-NTT (gg_kzg_to_lagrange_g1) and the whole
gg_plonk_setup, against the accumulate kernel's rate and the parent's route.

    python tools/bench_plonk_setup.py [--ecntt-log-n 16 20 22] [--setup-log-n 20 22] [--parent-log-n 20]
                                      [--bench-json FILE] [--out profiles/r09_plonk_setup.md]

The driver starts every measured step as a fresh child process under its own
`timeout` and stops at the first one that fails:
  ecntt   gg_kzg_to_lagrange_g1 on device buffers, both curves: one warm-up,
          then --reps timed calls (min and median);
  setup   gnark_amd.plonk_prover.SetupData by phase (gg_plonk_setup_timings) on a
          random sparse R1CS of 2^log_n - 3 constraints and 3 public inputs
          (BLS12-381), Lagrange SRS computed by the EC-NTT; then one key build
          (gg_plonk_setup_pk: the host bounce and the existing builder);
  parent  the parent commit's route to the scalar half of the same key shape:
          tests/plonk_circuits.Circuit.selectors / permutation / s_polys on the
          host, then ProvingKey(basis="lagrange").  Its permutation is NOT gnark's
          (unused slots are fixed points, the link direction differs), so the
          two keys differ: the times are comparable, the bytes are not;
  accum   the BN254 G1 bucket accumulation (k_accum_range) of a 2^22 MSM by the
          library's event profile: mixed additions per second, the yardstick the
          EC-NTT's field-multiplication rate is set against.  --bench-json takes the
          JSON line of `python bench.py --full` of the same session and adds its
          roofline entry (units x windows / kernel ms) beside it.
The points are [s]G for random s (a ceremony SRS is only points; the transform
does not care which).  The point-operation counts come from the recoding: per
multiplied butterfly 257 doublings and 6 additions (table included) plus one
addition per non-zero signed 4-bit digit of the twiddle, and two additions per
butterfly.  A further child
times the transform with the table-free non-adjacent form forced into every
stage (GG_ECNTT_MUL=naf) beside the library's 4-bit windows."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnark-fork_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# field multiplications per point operation (curve.cuh): dbl-2008-s-1 6M + 3S,
# add-2008-s 12M + 2S, madd-2008-s 8M + 2S
MUL_DBL, MUL_ADD, MUL_MADD = 9, 14, 10
# hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on csrc/ecntt.hip
RESOURCES = {("bn254", "non-adjacent form"): dict(vgpr=153, agpr=0, scratch=0, occupancy=3, block=128),
             ("bn254", "4-bit windows"): dict(vgpr=169, agpr=0, scratch=0, occupancy=2, block=128),
             ("bls12-381", "non-adjacent form"): dict(vgpr=225, agpr=0, scratch=0, occupancy=2, block=128),
             ("bls12-381", "4-bit windows"): dict(vgpr=231, agpr=0, scratch=0, occupancy=2, block=128)}


def _random_points(curve, count, seed):
    """count affine points [s]G, s random below 2^248 (device comb), as host bytes"""
    import numpy as np
    from gnark_amd import msm
    from plonk_circuits import FIELDS
    F = FIELDS[curve]
    s = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    s[:, 31] = 0  # < 2^248 < r: a valid Montgomery residue of some scalar
    group = msm.BLS12_381_G1 if curve == "bls12-381" else msm.G1
    return msm.batch_scalar_mul(group, F.g1_to_bytes(F.cv.G1), s.tobytes(), count)


def step_ecntt(curve, log_n, reps, mul=None):
    if mul:
        os.environ["GG_ECNTT_MUL"] = mul  # read by the library at every call
    from gnark_amd import kzg
    from gnark_amd._lib import DeviceBuffer, check, lib
    src = DeviceBuffer.from_host(_random_points(curve, 1 << log_n, log_n))
    dst = DeviceBuffer(src.nbytes)
    ms = []
    for _ in range(reps + 1):
        check(lib.gg_synchronize())
        t0 = time.perf_counter()
        kzg.to_lagrange_g1(src, log_n, curve=curve, out=dst)  # returns after its stream wait
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(step="ecntt", curve=curve, log_n=log_n, mul=mul or "windows", warmup_ms=ms[0], min_ms=min(ms[1:]),
                median_ms=statistics.median(ms[1:]))


def _random_system(log_n, seed=7):
    import numpy as np
    from gnark_amd import fr
    n_cons, nbp = (1 << log_n) - 3, 3
    rng = np.random.default_rng(seed)
    n_wires = n_cons + 8
    wires = rng.integers(0, n_wires, size=3 * n_cons, dtype=np.uint32)
    wires[rng.random(3 * n_cons) < 0.2] = 0  # wire 0 (and the padding) makes one long cycle
    qidx = rng.integers(0, 64, size=5 * n_cons, dtype=np.uint32)
    coeffs = b"".join(fr.bls_fr_mont(int(k)) for k in rng.integers(1, 1 << 62, size=64))
    return n_wires, nbp, wires, qidx, coeffs


def step_setup(log_n, reps):
    from gnark_amd import plonk_prover as pp
    system = _random_system(log_n)
    kzg_g1 = _random_points("bls12-381", (1 << log_n) + 3, 100 + log_n)
    runs, sd = [], None
    for _ in range(reps + 1):
        if sd is not None:
            sd.close()
        t0 = time.perf_counter()
        sd = pp.SetupData(*system, kzg_g1, None, (), "bls12-381")
        wall = 1e3 * (time.perf_counter() - t0)
        t = sd.timings()
        t["python_wall"] = wall
        runs.append(t)
    t0 = time.perf_counter()
    pk = sd.proving_key()
    pk_wall = 1e3 * (time.perf_counter() - t0)
    t = sd.timings()
    pk.close()
    sd.close()
    keys = [k for k in runs[0] if k not in ("pk_host_bounce", "pk_build")]
    return dict(step="setup", log_n=log_n, phases={k: dict(min=min(r[k] for r in runs[1:]),
                                                           median=statistics.median(r[k] for r in runs[1:]))
                                                   for k in keys},
                pk_host_bounce_ms=t["pk_host_bounce"], pk_build_ms=t["pk_build"], pk_wall_ms=pk_wall)


def step_parent(log_n):
    from gnark_amd import plonk_prover as pp
    from plonk_circuits import Circuit
    t = {}
    t0 = time.perf_counter()
    circ = Circuit(log_n, 5, nb_public=3)
    t["circuit_rows_host"] = 1e3 * (time.perf_counter() - t0)
    pts = _random_points("bls12-381", (1 << log_n) + 3, 100 + log_n)
    t0 = time.perf_counter()
    sel, qcp = circ.selectors()
    t["selectors_host"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    perm = circ.permutation()
    t["permutation_host"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    s123 = circ.s_polys(perm, circ.F.cv.omega(circ.n), circ.F.cv.fr_gen)
    t["s_polys_host"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    pk = pp.ProvingKey(log_n, pts, pts[:96 << log_n], *sel, *s123, perm.tobytes(), qcp=qcp, nb_public=3,
                       basis="lagrange")
    t["proving_key_lagrange_basis"] = 1e3 * (time.perf_counter() - t0)
    pk.close()
    return dict(step="parent", log_n=log_n, ms=t)


def step_accum(log_n, reps):
    import numpy as np
    from gnark_amd import _lib, msm
    n = 1 << log_n
    base = msm.MsmBase(msm.G1, _random_points("bn254", n, 3), n)
    sc = np.random.default_rng(4).integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x0f
    sc = sc.tobytes()
    base.msm_jac(sc, n)  # warm-up
    _lib.profile_enable(True)
    for _ in range(reps):
        base.msm_jac(sc, n)
    tot, cnt, units = _lib.profile_get("msm_accum")
    _lib.profile_enable(False)
    _n, c, windows = base.info()
    ms = tot / cnt
    return dict(step="accum", log_n=log_n, window_bits=c, windows=windows, launches=cnt, avg_ms=ms,
                units_per_launch=units / cnt, madds_per_s=units / cnt * windows / (ms * 1e-3))


# ------------------------------------------------------------ operation counts
_C8 = int("8" * 64, 16)
_C1 = int("1" * 65, 16)


def _naf_adds(t):
    return bin((3 * t) ^ t).count("1")


def _window_adds(t):
    """non-zero digits of the signed 4-bit recoding (nibbles of t + 0x88..8 that are
    not 8; the carry nibble as it is) + the 6 additions of the table 3P..8P"""
    z = (t + _C8) ^ _C8
    return bin((z | z >> 1 | z >> 2 | z >> 3) & _C1).count("1") + 6


def op_counts(curve, log_n):
    """(doublings, additions) the stage kernels execute for an input without
    infinities, from the recoding of every twiddle they multiply by: windows
    (256 doublings + 1 for the table) in every stage but the last, whose single
    product, like out[0]'s, goes by the non-adjacent form (256 doublings)"""
    from plonk_circuits import FIELDS
    cv = FIELDS[curve].cv
    R, n, nh = cv.R, 1 << log_n, 1 << (log_n - 1)
    w, ninv = pow(cv.omega(n), -1, R), pow(n, -1, R)
    wt = [0] * nh   # additions of the product by w^j
    wt0 = [0] * nh  # ... by w^j / n (block 0)
    t = 1
    for j in range(nh):
        wt[j] = _window_adds(t)
        wt0[j] = _window_adds(t * ninv % R)
        t = t * w % R
    dbl = add = 0
    for s in range(log_n - 1):
        blocks = 1 << s
        idx = range(0, nh, blocks)                      # w^(j 2^s), j < half
        mult = len(idx) - 1                             # j = 0 is skipped outside block 0
        dbl += 257 * ((blocks - 1) * mult + len(idx))   # block 0 multiplies j = 0 too
        add += (blocks - 1) * sum(wt[i] for i in idx if i) + sum(wt0[i] for i in idx)
    dbl += 2 * 256                                       # the last stage's block 0, out[0] / n
    add += 2 * _naf_adds(ninv)
    add += 2 * nh * log_n                                # a + b and a - b of every butterfly
    return dbl, add


# ------------------------------------------------------------ driver
def child(args):
    if args.child == "ecntt":
        r = step_ecntt(args.curve, args.log_n, args.reps, args.mul)
    elif args.child == "setup":
        r = step_setup(args.log_n, args.reps)
    elif args.child == "parent":
        r = step_parent(args.log_n)
    else:
        r = step_accum(args.log_n, args.reps)
    print("RESULT " + json.dumps(r), flush=True)


def run_child(step, limit, *extra):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", step] + \
        [str(x) for x in extra]
    print("+ " + " ".join(cmd[4:]), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-4000:])
        raise SystemExit("step %s failed with status %d: stopping" % (step, p.returncode))
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    r = json.loads(line[7:])
    print("  " + json.dumps(r), flush=True)
    return r


def write_note(path, res, bench_roofline):
    acc = res["accum"]
    acc_mul = acc["madds_per_s"] * MUL_MADD
    L = ["# PlonK Setup on the GPU: EC-NTT and setup phases (tools/bench_plonk_setup.py)", "",
         "One MI355X.  Every row is a fresh process; min and median of %d calls after one warm-up." % res["reps"],
         "Field multiplications per point operation: doubling %d, addition %d, mixed addition %d." %
         (MUL_DBL, MUL_ADD, MUL_MADD), "",
         "## Yardstick: the bucket accumulation", "",
         "`k_accum_range<Fp>` of a standalone 2^%d BN254 G1 MSM (window %d bits, %d windows), the library's event "
         "profile over %d launches: %.3f ms per launch, %.3g mixed additions/s = **%.3g 256-bit field "
         "multiplications/s**." % (acc["log_n"], acc["window_bits"], acc["windows"], acc["launches"], acc["avg_ms"],
                                   acc["madds_per_s"], acc_mul)]
    if bench_roofline:
        r = bench_roofline
        rate = r["units_per_launch"] * r["windows"] / (r["kernel_avg_ms"] * 1e-3)
        L.append("`python bench.py --full` of the same session, roofline section: %.3g units x %d windows in %.3f ms "
                 "= %.3g mixed additions/s = %.3g field multiplications/s." %
                 (r["units_per_launch"], r["windows"], r["kernel_avg_ms"], rate, rate * MUL_MADD))
    else:
        L.append("(`python bench.py --full` was not run in this session; the figure above is the same kernel timed "
                 "by the same event profile on a standalone MSM.)")
    L += ["", "## EC-NTT (gg_kzg_to_lagrange_g1, device in, device out)", "",
          "| curve | n | min ms | median ms | doublings | additions | field mult. | mult./s | / accumulate |",
          "|---|---|---|---|---|---|---|---|---|"]
    for e in res["ecntt"]:
        dbl, add = e["ops"]
        mul = dbl * MUL_DBL + add * MUL_ADD
        rate = mul / (e["min_ms"] * 1e-3)
        L.append("| %s | 2^%d | %.1f | %.1f | %.4g | %.4g | %.4g | %.3g | %.2f |" %
                 (e["curve"], e["log_n"], e["min_ms"], e["median_ms"], dbl, add, mul, rate, rate / acc_mul))
    L += ["", "Reading the ratio: a butterfly is one thread, so 2^16 points are 2^15 threads = 512 waves for the "
          "1024 SIMDs of the device, each a serial chain of 256 doublings: the small size is bound by that latency, "
          "not by throughput.  At 2^20 and above the grid fills the device at the occupancy below.  With the "
          "non-adjacent form, stages with at least 64 blocks run with one twiddle per wave (no divergence), but the "
          "first six stages have a different twiddle in every lane, so a wave executes the addition at nearly every "
          "one of the 256 digits although each lane needs it at a third of them; signed 4-bit windows add at the same 65 places in every lane, "
          "and measured faster in the other stages too (table below), so every stage uses them.  The counts here "
          "are theirs: 257 doublings and 6 additions for the table plus one per non-zero digit, for every product.",
          "", "BLS12-381 multiplications are 12-limb (381-bit), the accumulate's are 8-limb (256-bit): about "
          "(12/8)^2 = 2.25x the multiply-adds each, so the BLS12-381 ratio understates the ALU work by that factor.",
          "", "Compiler figures of `k_stage` (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):", "",
          "| curve | twiddle product | VGPRs | AGPRs | scratch B/lane | waves/SIMD | block |",
          "|---|---|---|---|---|---|---|"]
    for (c, m), r in RESOURCES.items():
        L.append("| %s | %s | %d | %d | %d | %d | %d |" % (c, m, r["vgpr"], r["agpr"], r["scratch"], r["occupancy"],
                                                          r["block"]))
    if res.get("variants"):
        auto = {(e["curve"], e["log_n"]): e for e in res["ecntt"]}
        L += ["", "The twiddle product, measured: the non-adjacent form in every stage (GG_ECNTT_MUL=naf, no table) "
              "against the library's signed 4-bit windows (8 table points per thread in HBM):", "",
              "| curve | n | non-adjacent form, min ms | 4-bit windows, min ms |", "|---|---|---|---|"]
        for e in res["variants"]:
            a = auto.get((e["curve"], e["log_n"]))
            L.append("| %s | 2^%d | %.1f | %s |" % (e["curve"], e["log_n"], e["min_ms"], "%.1f" % a["min_ms"] if a else "-"))
    L += ["", "## gg_plonk_setup by phase (BLS12-381, random sparse R1CS, 3 public inputs, Lagrange SRS computed)", ""]
    names = list(res["setup"][0]["phases"]) if res["setup"] else []
    L += ["| phase | " + " | ".join("2^%d min / median ms" % s["log_n"] for s in res["setup"]) + " |",
          "|---|" + "---|" * len(res["setup"])]
    for k in names:
        L.append("| %s | " % k + " | ".join("%.1f / %.1f" % (s["phases"][k]["min"], s["phases"][k]["median"])
                                             for s in res["setup"]) + " |")
    L += ["", "Key build through gg_plonk_setup_pk (once per size): the results are copied to pinned host memory "
          "and handed to the existing builder, whose body is unchanged.", "",
          "| n | host bounce ms | builder ms (MSM tables, commitTrace, domains) |", "|---|---|---|"]
    for s in res["setup"]:
        L.append("| 2^%d | %.1f | %.1f |" % (s["log_n"], s["pk_host_bounce_ms"], s["pk_build_ms"]))
    if res["parent"]:
        p = res["parent"]
        mine = next((s for s in res["setup"] if s["log_n"] == p["log_n"]), None)
        L += ["", "## The parent's route to the scalar half at 2^%d (same run)" % p["log_n"], "",
              "tests/plonk_circuits.Circuit on the host, then ProvingKey(basis=\"lagrange\").  **The parent's "
              "permutation is not gnark's** (unused slots are fixed points there, wire 0's cycle in gnark; the "
              "link direction differs), so its key is not the key gnark's Setup makes; only the times compare.", "",
              "| step | ms |", "|---|---|"]
        for k, v in p["ms"].items():
            L.append("| %s | %.1f |" % (k, v))
        if mine:
            scalar = sum(mine["phases"][k]["min"] for k in ("validate_upload", "trace", "permutation", "s_gather",
                                                            "inverse_ntts"))
            L += ["", "This change at 2^%d: validation + upload, trace, permutation, S gather and inverse NTTs "
                  "together %.1f ms; the key build (bounce + builder) %.1f ms." %
                  (p["log_n"], scalar, mine["pk_host_bounce_ms"] + mine["pk_build_ms"])]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--curve", default="bls12-381")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mul", default=None, help="ecntt child: GG_ECNTT_MUL (naf; default: the library's windows)")
    ap.add_argument("--variants-log-n", type=int, default=20, help="size of the naf / window comparison (0: skip)")
    ap.add_argument("--ecntt-log-n", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--setup-log-n", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--parent-log-n", type=int, default=20, help="0: skip the parent's route")
    ap.add_argument("--bench-json", default=None, help="the JSON line of `python bench.py --full` (roofline)")
    ap.add_argument("--save", default=None, help="keep the measurements as JSON")
    ap.add_argument("--load", default=None, help="measurements of an earlier --save of this session: only "
                                                 "rewrite the note (with --bench-json)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_plonk_setup.md"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.load:
        with open(args.load) as f:
            res = json.load(f)
        for e in res["ecntt"]:
            e["ops"] = op_counts(e["curve"], e["log_n"])
    else:
        res = measure(args)
    if args.save:
        with open(args.save, "w") as f:
            json.dump(res, f)
    roofline = None
    if args.bench_json:
        with open(args.bench_json) as f:
            for line in f:
                if line.startswith("{") and '"roofline"' in line:
                    roofline = json.loads(line)["roofline"]
    write_note(args.out, res, roofline)
    print(json.dumps(res))


def measure(args):
    common = ["--reps", args.reps]
    res = dict(reps=args.reps, ecntt=[], setup=[], parent=None)
    res["accum"] = run_child("accum", 300, "--log-n", 22, *common)
    for log_n in args.ecntt_log_n:
        for curve in ("bn254", "bls12-381"):
            e = run_child("ecntt", 300, "--curve", curve, "--log-n", log_n, *common)
            e["ops"] = op_counts(curve, log_n)
            res["ecntt"].append(e)
    res["variants"] = []
    if args.variants_log_n:
        for curve in ("bn254", "bls12-381"):
            for mul in ("naf",):
                res["variants"].append(run_child("ecntt", 300, "--curve", curve, "--log-n", args.variants_log_n,
                                                 "--mul", mul, *common))
    for log_n in args.setup_log_n:
        res["setup"].append(run_child("setup", 600, "--log-n", log_n, *common))
    if args.parent_log_n:
        res["parent"] = run_child("parent", 600, "--log-n", args.parent_log_n)
    return res


if __name__ == "__main__":
    main()

"""Groth16 Setup on the GPU against what the tree had before it, for the MiMC
shapes of tests/test_gpu_groth16_size.py (rounds 85, one public input, that
file's toxic waste) at 2^20 and 2^24 constraints.

    python tools/bench_setup.py [--log-n 20 24] [--reps 3] [--out profiles/r08_groth16_setup.md]

The driver starts every measured step as a fresh child process under its own
`timeout` and stops at the first one that fails:
  gpu     gnark_amd.groth16.setup_device by phase (gg_groth16_setup_timings:
          transpose, Lagrange table, accumulate, K / Z / compaction, G1 points,
          G2 points) and the read-back of every part; one warm-up setup of the
          same size first, then --reps timed ones (min and median reported);
  parent  what the parent commit does for the same key: coracle.key_scalars on
          16 threads, then the five msm.batch_scalar_mul calls of `_instance`.
Both children write a SHA-256 per key part; the driver asserts that the two
keys are byte-identical part by part (the one 2^24 correctness check: not in
pytest) and writes the table.  The accumulate kernel's launches, threads and
bytes per term are computed from the counts the library reports."""
import argparse
import hashlib
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

TW = dict(tau=0x1DEA5EED1234567, alpha=0xA1FA0001, beta=0xBE7A0002, delta=0xDE17A0003)
GAMMA = 0x6A77A0004  # the parent's key has no vk: gamma only enters vk.K / [gamma]2
ROUNDS = 85
PARTS = ("g1_A", "g1_B", "g1_K", "g1_Z", "g2_B", "alpha1", "beta1", "delta1", "beta2", "delta2", "infA", "infB")


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def step_gpu(log_n, reps):
    import numpy as np  # noqa: F401
    from gnark_amd import groth16, _lib as L
    from test_gpu_solver import mimc_csr
    chains = 1 << (log_n - 8)
    m = mimc_csr(chains, ROUNDS, 1)
    tw = groth16.ToxicWaste(TW["tau"], TW["alpha"], TW["beta"], GAMMA, TW["delta"])
    args = (m["nb_public"], m["nw"], m["off"], m["wires"], m["coef"], m["table"])
    runs, digests, info = [], None, None
    for it in range(reps + 1):  # the first one warms up (code objects, allocator)
        t0 = time.perf_counter()
        res = groth16.setup_device(*args, toxic_waste=tw)
        wall = 1e3 * (time.perf_counter() - t0)
        t = res.timings()
        g1b, g2b = 64, 128
        t1 = time.perf_counter()
        parts = dict(
            g1_A=res.read(L.GG_SETUP_G1_A, res.nA * g1b), g1_B=res.read(L.GG_SETUP_G1_B, res.nB * g1b),
            g1_K=res.read(L.GG_SETUP_G1_K, res.nK * g1b), g1_Z=res.read(L.GG_SETUP_G1_Z, res.nZ * g1b),
            g2_B=res.read(L.GG_SETUP_G2_B, res.nB * g2b), alpha1=res.read(L.GG_SETUP_ALPHA1, g1b),
            beta1=res.read(L.GG_SETUP_BETA1, g1b), delta1=res.read(L.GG_SETUP_DELTA1, g1b),
            beta2=res.read(L.GG_SETUP_BETA2, g2b), delta2=res.read(L.GG_SETUP_DELTA2, g2b),
            infA=res.read(L.GG_SETUP_INFINITY_A, m["nw"]), infB=res.read(L.GG_SETUP_INFINITY_B, m["nw"]))
        t["readback"] = 1e3 * (time.perf_counter() - t1)
        t["setup_call"] = wall
        info = dict(acc_chunk=res.acc_chunk, acc_launches=res.acc_launches, nA=res.nA, nB=res.nB, nK=res.nK,
                    nZ=res.nZ, n_wires=m["nw"], n_constraints=m["ncons"])
        res.close()
        if it == 0:
            digests = {k: _sha(v) for k, v in parts.items()}
        else:
            runs.append(t)
        del parts
    return dict(step="gpu", log_n=log_n, runs=runs, info=info, digests=digests)


def step_parent(log_n, reps):
    import bn254_oracle as o
    import coracle
    from gnark_amd import msm
    chains = 1 << (log_n - 8)
    cr = coracle.MimcR1CS(chains, ROUNDS, 1)
    f = lambda v: o.fr_to_bytes(v % o.R)
    tw = {k: f(v) for k, v in TW.items()}
    g1, g2 = o.g1_to_bytes(o.G1_GEN), o.g2_to_bytes(o.G2_GEN)
    msm.batch_scalar_mul(msm.G1, g1, tw["alpha"] * 4096, 4096)  # warm-up of both combs
    msm.batch_scalar_mul(msm.G2, g2, tw["alpha"] * 4096, 4096)
    runs, digests = [], None
    for it in range(reps):
        t0 = time.perf_counter()
        ks = cr.key_scalars(log_n, tw["tau"], tw["alpha"], tw["beta"], tw["delta"], 16)
        t_ks = 1e3 * (time.perf_counter() - t0)
        t1 = time.perf_counter()
        pts = dict(g1_A=msm.batch_scalar_mul(msm.G1, g1, ks["A"], len(ks["A"]) // 32),
                   g1_B=msm.batch_scalar_mul(msm.G1, g1, ks["B"], len(ks["B"]) // 32),
                   g1_Z=msm.batch_scalar_mul(msm.G1, g1, ks["Z"], len(ks["Z"]) // 32),
                   g1_K=msm.batch_scalar_mul(msm.G1, g1, ks["K"], len(ks["K"]) // 32),
                   g2_B=msm.batch_scalar_mul(msm.G2, g2, ks["B"], len(ks["B"]) // 32))
        t_pts = 1e3 * (time.perf_counter() - t1)
        runs.append(dict(key_scalars_16_threads=t_ks, five_batch_scalar_mul=t_pts))
        if digests is None:
            pts.update(alpha1=msm.batch_scalar_mul(msm.G1, g1, tw["alpha"], 1),
                       beta1=msm.batch_scalar_mul(msm.G1, g1, tw["beta"], 1),
                       delta1=msm.batch_scalar_mul(msm.G1, g1, tw["delta"], 1),
                       beta2=msm.batch_scalar_mul(msm.G2, g2, tw["beta"], 1),
                       delta2=msm.batch_scalar_mul(msm.G2, g2, tw["delta"], 1), infA=ks["infA"], infB=ks["infB"])
            digests = {k: _sha(v) for k, v in pts.items()}
        del ks, pts
    cr.close()
    return dict(step="parent", log_n=log_n, runs=runs, digests=digests)


def _stat(runs, key):
    v = [r[key] for r in runs]
    return min(v), statistics.median(v)


def _table(results):
    out = ["| step | " + " | ".join("2^%d min / median ms" % ln for ln in sorted(results)) + " |",
           "|---|" + "---|" * len(results)]
    gpu_keys = [("transpose", "transpose (host checks, upload, count / scan / fill)"), ("lagrange", "Lagrange table"),
                ("accumulate", "accumulate (all rounds, with their scans)"),
                ("accumulate_kernels", "  of which the accumulate kernels (device events)"),
                ("kz", "K, Z and compaction"), ("g1", "G1 points"), ("g2", "G2 points"),
                ("setup_call", "GPU Setup, the whole call"), ("readback", "read-back of every part")]
    for key, label in gpu_keys:
        out.append("| %s | " % label + " | ".join("%.1f / %.1f" % _stat(results[ln]["gpu"]["runs"], key)
                                                 for ln in sorted(results)) + " |")
    for key, label in (("key_scalars_16_threads", "parent: coracle.key_scalars, 16 threads"),
                       ("five_batch_scalar_mul", "parent: the five batch_scalar_mul calls")):
        out.append("| %s | " % label + " | ".join("%.1f / %.1f" % _stat(results[ln]["parent"]["runs"], key)
                                                 for ln in sorted(results)) + " |")
    out.append("")
    for ln in sorted(results):
        g = results[ln]["gpu"]
        r = g["runs"][0]
        terms, thr = r["terms"], r["accumulate_threads"]
        amin, _ = _stat(g["runs"], "accumulate_kernels")
        # per term: 8-B entry + 32-B L gather (the coefficient table stays in cache); per thread:
        # one 32-B sum written, read once more by the next round when it is a partial (upper bound)
        bpt = 40.0 + 64.0 * thr / terms
        out.append("2^%d accumulate: %d terms, chunk %d, %d launches, %d threads, <= %.1f B moved per term, "
                   "%.2f ms in the kernels (%.1f GB/s of that traffic)."
                   % (ln, terms, g["info"]["acc_chunk"], g["info"]["acc_launches"], thr, bpt, amin,
                      bpt * terms / amin / 1e6))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_groth16_setup.md"))
    ap.add_argument("--step", choices=["gpu", "parent"])
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step:  # a child: one step at one size
        res = (step_gpu if a.step == "gpu" else step_parent)(a.log_n[0], a.reps)
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    results = {}
    tmp = os.path.join(os.path.dirname(a.out), ".bench_setup")
    os.makedirs(tmp, exist_ok=True)
    for ln in a.log_n:
        results[ln] = {}
        for step in ("gpu", "parent"):
            js = os.path.join(tmp, "%s_%d.json" % (step, ln))
            limit = 120 if ln <= 20 else 420
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--log-n", str(ln), "--reps", str(a.reps), "--json", js]
            print("+", " ".join(cmd), flush=True)
            rc = subprocess.call(cmd)
            if rc != 0:  # nothing more on the GPU after a failed step
                sys.exit("step %s at 2^%d ended with status %d" % (step, ln, rc))
            results[ln][step] = json.load(open(js))
            os.remove(js)
        dg, dp = results[ln]["gpu"]["digests"], results[ln]["parent"]["digests"]
        bad = [k for k in PARTS if dg[k] != dp[k]]
        assert not bad, "2^%d: the GPU Setup's key differs from the parent's in %s" % (ln, bad)
        print("2^%d: both keys byte-identical in %s" % (ln, ", ".join(PARTS)), flush=True)
    os.rmdir(tmp)
    text = ("# Groth16 Setup on the GPU (tools/bench_setup.py)\n\n"
            "MiMC shape (rounds 85, one public input), BN254, one MI355X; %d timed runs per step after one\n"
            "warm-up, each step a process of its own.  The two keys were byte-identical part by part\n"
            "(SHA-256 of A, B, K, Z, G2.B, alpha, beta, delta, both infinity masks) at every size listed.\n\n"
            % a.reps) + _table(results) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

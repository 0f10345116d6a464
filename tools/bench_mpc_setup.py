"""Groth16 keys from a powers-of-tau SRS on the GPU (gnark_amd.mpcsetup), phase by
phase, with gg_groth16_setup of the same circuit in the same process beside it
for scale.  MiMC-shaped R1CS (rounds 85, one public input: the shape of
tools/bench_setup.py) and a single-party trapdoor SRS of exactly the domain.

    python tools/bench_mpc_setup.py [--curve bn254 bls12-381] [--log-n 16 20] [--reps 2]
                                    [--out profiles/r15_groth16_mpc_setup.md]

2^22 and 2^24 are options, not defaults (--log-n 22 24).  The driver starts one
child process per (curve, size) under its own `timeout` and stops at the first
one that fails.  A child builds the SRS (not timed: a ceremony hands it over),
warms up at 2^10, then times --reps init_phase2 calls (min reported, by the
library's own phases: gg_groth16_setup_timings), one contribution after each,
and --reps gg_groth16_setup calls.  It asserts that the key extracted after the
contribution delta equals, part by part (SHA-256), the key gg_groth16_setup
makes from (tau, alpha, beta, 1, delta)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnark-fork_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAU, ALPHA, BETA, DELTA = 0x1DEA5EED1234567, 0xA1FA0001, 0xBE7A0002, 0xDE17A0003
ROUNDS = 85
PHASES = [("upload_check", "SRS upload and point checks"), ("transpose", "transpose, coefficient classes, general-term list"),
          ("ecntt_tau_g1", "EC-NTT tau_g1"), ("ecntt_alpha_tau_g1", "EC-NTT alpha_tau_g1"),
          ("ecntt_beta_tau_g1", "EC-NTT beta_tau_g1"), ("ecntt_tau_g2", "EC-NTT tau_g2 (G2)"),
          ("accumulate", "accumulate, the three runs with their scans"),
          ("general_abc", "  general terms x [L]1 (device events)"), ("accumulate_abc", "  rounds -> A, B1, C"),
          ("general_k", "  general terms x [beta L]1, [alpha L]1"), ("accumulate_k", "  rounds -> bA, aB"),
          ("general_g2", "  general terms x [L]2"), ("accumulate_g2", "  rounds -> G2.B"),
          ("z", "Z"), ("kz", "K, flags, compaction and Z"), ("normalise", "normalise to affine, every array"),
          ("init_phase2", "init_phase2, the whole call"), ("contribute", "one contribution"),
          ("extract_keys", "extract_keys (read-back)"), ("setup", "gg_groth16_setup, the whole call"),
          ("setup_read", "gg_groth16_setup read-back")]


def _circuit(curve, log_n):
    from gnark_amd import fr
    from test_gpu_solver import mimc_csr
    m = mimc_csr(1 << (log_n - 8), ROUNDS, 1)
    mod = fr.R if curve == "bn254" else fr.BLS_R
    table = [1] + [(-(r * 7 + 3)) % mod for r in range(ROUNDS)]  # mimc_csr's table over this curve's field
    return m, (m["nb_public"], m["nw"], m["off"], m["wires"], m["coef"], table)


def _digests(keys):
    import dataclasses
    out = {}
    for k in keys:
        for f in dataclasses.fields(k):
            v = getattr(k, f.name)
            if isinstance(v, (bytes, bytearray)):
                out[type(k).__name__ + "." + f.name] = hashlib.sha256(bytes(v)).hexdigest()
    return out


def child(curve, log_n, reps):
    from gnark_amd import fr, groth16, mpcsetup
    mod = fr.R if curve == "bn254" else fr.BLS_R
    tw = groth16.ToxicWaste(TAU % mod, ALPHA, BETA, 1, DELTA)
    for ln in (10, log_n):  # the first size warms up (code objects, allocator)
        m, args = _circuit(curve, ln)
        assert m["ncons"] <= 1 << ln
        srs = mpcsetup.srs_from_trapdoor(ln, TAU % mod, ALPHA, BETA, curve)
        runs, dg = [], None
        for _ in range(reps if ln == log_n else 1):
            t0 = time.perf_counter()
            p2 = mpcsetup.init_phase2(*args, srs)
            wall = 1e3 * (time.perf_counter() - t0)
            p2.contribute(DELTA)
            t1 = time.perf_counter()
            keys = p2.extract_keys()
            t = p2.timings()
            t["extract_keys"] = 1e3 * (time.perf_counter() - t1)
            t["init_phase2"] = wall
            info = dict(acc_chunk=p2.acc_chunk, acc_launches=p2.acc_launches, n_wires=m["nw"], n_constraints=m["ncons"])
            p2.close()
            dg = _digests(keys)
            del keys
            t0 = time.perf_counter()
            res = groth16.setup_device(*args, toxic_waste=tw, curve=curve)
            t["setup"] = 1e3 * (time.perf_counter() - t0)
            t1 = time.perf_counter()
            want = groth16.read_keys(res, m["nw"], m["nb_public"])
            t["setup_read"] = 1e3 * (time.perf_counter() - t1)
            res.close()
            dw = _digests(want)
            del want
            bad = [k for k in dw if dw[k] != dg[k]]
            assert not bad, "%s 2^%d: the key from the SRS differs from gg_groth16_setup's in %s" % (curve, ln, bad)
            runs.append(t)
    return dict(curve=curve, log_n=log_n, runs=runs, info=info, parts=sorted(dg))


def _table(results):
    cols = sorted(results)
    out = ["| phase, ms (min of the runs) | " + " | ".join("%s 2^%d" % c for c in cols) + " |", "|---|" + "---|" * len(cols)]
    for key, label in PHASES:
        out.append("| %s | " % label + " | ".join("%.1f" % min(r[key] for r in results[c]["runs"]) for c in cols) + " |")
    out.append("")
    for c in cols:
        r, i = results[c]["runs"][0], results[c]["info"]
        out.append("%s 2^%d: %d constraints, %d wires, %d terms of which %d general; chunk %d, %d accumulation launches, "
                   "%d threads." % (c[0], c[1], i["n_constraints"], i["n_wires"], r["terms"], r["general_terms"],
                                    i["acc_chunk"], i["acc_launches"], r["accumulate_threads"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", nargs="+", default=["bn254", "bls12-381"], choices=["bn254", "bls12-381"])
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_groth16_mpc_setup.md"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.child:
        res = child(a.curve[0], a.log_n[0], a.reps)
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    results = {}
    tmp = os.path.join(os.path.dirname(os.path.abspath(a.out)), ".bench_mpc_setup")
    os.makedirs(tmp, exist_ok=True)
    for ln in a.log_n:
        for curve in a.curve:
            js = os.path.join(tmp, "%s_%d.json" % (curve, ln))
            limit = 150 if ln <= 16 else 420 if ln <= 20 else 1100
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", "--curve",
                   curve, "--log-n", str(ln), "--reps", str(a.reps), "--json", js]
            print("+", " ".join(cmd), flush=True)
            rc = subprocess.call(cmd)
            if rc != 0:  # nothing more on the GPU after a failed step
                sys.exit("%s at 2^%d ended with status %d" % (curve, ln, rc))
            results[(curve, ln)] = json.load(open(js))
            os.remove(js)
            print("%s 2^%d: the key from the SRS equals gg_groth16_setup's in %d parts" %
                  (curve, ln, len(results[(curve, ln)]["parts"])), flush=True)
    os.rmdir(tmp)
    text = ("# Groth16 keys from a powers-of-tau SRS (tools/bench_mpc_setup.py)\n\n"
            "MiMC shape (rounds 85, one public input), trapdoor SRS of exactly the domain, host buffers in, one\n"
            "MI355X; %d timed runs per size after a warm-up at 2^10, one process per column.  check_points on.\n"
            "In every column the key extracted after one contribution was byte-identical, part by part (SHA-256),\n"
            "to the key gg_groth16_setup made from (tau, alpha, beta, 1, delta) in the same process.\n\n"
            % a.reps) + _table(results) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

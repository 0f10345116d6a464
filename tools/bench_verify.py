"""Groth16 Verify on the GPU: proofs per second for batches under one key.

    python tools/bench_verify.py [--n 1 64 1024 16384] [--nb-public 2 64] [--reps 3]
                                 [--resources-json FILE] [--out profiles/r10_groth16_verify.md]
    python tools/bench_verify.py --curve both --nb-public 2 [--out profiles/r13_bls12_381_groth16_verify.md]

--curve bn254 (the default) is the BN254 report.  --curve bls12-381 / both
measures the BLS12-381 verifier (tests/bls_groth16_ref.py instances), with
`both` beside the BN254 verifier in the same process, and adds the step
  endo       gg_g{1,2}_check_endo_bls12_381 against gg_g{1,2}_check_bls12_381 on
             the same 16384 valid points, min of 3 calls after a warm-up.

Synthetic BN254 instances (tests/pairing_ref.py: a key from discrete logs, 64
distinct valid proofs tiled to the batch size).  The driver starts every
measured step as a fresh child process under its own `timeout` and stops at
the first one that fails:
  gpu        gnark_amd gg_groth16_verify_batch on packed host buffers (uploads
             and the status read-back included), one warm-up call per size and
             then --reps timed ones, the min reported; every status must be OK,
             and one corrupted proof per batch must be the only failure;
  oracle     oracle/bn254_oracle.py:verify for one proof on this CPU, the only
             baseline the project has;
  resources  the code-object figures of groth16_verify.hip's kernels (VGPRs, scratch,
             LDS, waves per SIMD) from the compiler's resource remarks; needs
             no GPU (--step resources --json FILE writes them, --resources-json
             FILE reuses them)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnark-fork_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DISTINCT = 64


def _instances(nb_public):
    import bn254_oracle as o
    import pairing_ref as pr
    key = pr.SyntheticKey(nb_public - 1, seed=1000 + nb_public)
    rng = o.SplitMix64(nb_public)
    wits = [[rng.fr() for _ in range(nb_public - 1)] for _ in range(DISTINCT)]
    proofs = [key.prove(w) for w in wits]
    return key, proofs, wits


def step_gpu(nb_public, sizes, reps):
    import ctypes
    import bn254_oracle as o
    import pairing_ref as pr
    from gnark_amd import groth16
    from gnark_amd._lib import check, lib, ptr
    key, proofs, wits = _instances(nb_public)
    t0 = time.perf_counter()
    vk = groth16.VerifyingKey(key.vk_data())
    t_key = 1e3 * (time.perf_counter() - t0)
    pb = [pr.proof_bytes(p) for p in proofs]
    wb = [o.fr_vec_to_bytes(w) for w in wits]
    bad = bytearray(pb[0])
    bad[192:256] = o.g1_to_bytes(o.g1_add(proofs[0].Krs, o.G1_GEN))
    rows = []
    for n in sizes:
        packed = bytearray(b"".join(pb[i % DISTINCT] for i in range(n)))
        wit = b"".join(wb[i % DISTINCT] for i in range(n))
        status = bytearray(n)
        times = []
        for it in range(reps + 1):  # the first call warms up (code objects, the key's buffers)
            t0 = time.perf_counter()
            check(lib.gg_groth16_verify_batch(vk.handle, n, ptr(packed), None, None, ptr(wit) if wit else None,
                                              ptr(status)))
            dt = time.perf_counter() - t0
            assert not any(status), "a valid proof was rejected at n = %d" % n
            if it:
                times.append(dt)
        packed[256 * (n - 1):256 * n] = bad if (n - 1) % DISTINCT == 0 else packed[256 * (n - 1):256 * n]
        if (n - 1) % DISTINCT == 0:
            check(lib.gg_groth16_verify_batch(vk.handle, n, ptr(packed), None, None, ptr(wit) if wit else None,
                                              ptr(status)))
            assert list(status) == [0] * (n - 1) + [3], "the corrupted proof was not the only failure"
        rows.append(dict(n=n, min_ms=1e3 * min(times), proofs_per_s=n / min(times)))
    vk.close()
    return dict(step="gpu", nb_public=nb_public, key_ms=t_key, rows=rows)


def _instances_bls(nb_public):
    import random
    import bls12_381_oracle as bo
    import bls_groth16_ref as gr
    key = gr.SyntheticKey(nb_public - 1, seed=1000 + nb_public)
    rng = random.Random(nb_public)
    wits = [[rng.randrange(bo.R) for _ in range(nb_public - 1)] for _ in range(DISTINCT)]
    proofs = [key.prove(w) for w in wits]
    return key, proofs, wits


def step_gpu_bls(nb_public, sizes, reps):
    import bls12_381_oracle as bo
    from gnark_amd import groth16
    from gnark_amd._lib import check, lib, ptr
    key, proofs, wits = _instances_bls(nb_public)
    t0 = time.perf_counter()
    vk = groth16.Bls12381VerifyingKey(key.vk_data())
    t_key = 1e3 * (time.perf_counter() - t0)
    gp = [p.gproof() for p in proofs]
    pb = [g.Ar + g.Bs + g.Krs for g in gp]
    wb = [bo.fr_vec_to_bytes(w) for w in wits]
    bad = pb[0][:288] + bo.g1_to_bytes(bo.g1_add(proofs[0].krs, bo.G1_GEN))
    fn = lib.gg_groth16_verify_batch_bls12_381
    status = bytearray(1)
    t0 = time.perf_counter()     # the first device batch: the upload and the window table of K[1:]
    check(fn(vk.handle, 1, ptr(pb[0]), None, None, ptr(wb[0]) if wb[0] else None, ptr(status)))
    t_first = 1e3 * (time.perf_counter() - t0)
    rows = []
    for n in sizes:
        packed = bytearray(b"".join(pb[i % DISTINCT] for i in range(n)))
        wit = b"".join(wb[i % DISTINCT] for i in range(n))
        status = bytearray(n)
        times = []
        for it in range(reps + 1):  # the first call warms up (the key's buffers)
            t0 = time.perf_counter()
            check(fn(vk.handle, n, ptr(packed), None, None, ptr(wit) if wit else None, ptr(status)))
            dt = time.perf_counter() - t0
            assert not any(status), "a valid proof was rejected at n = %d" % n
            if it:
                times.append(dt)
        if (n - 1) % DISTINCT == 0:
            packed[384 * (n - 1):384 * n] = bad
            check(fn(vk.handle, n, ptr(packed), None, None, ptr(wit) if wit else None, ptr(status)))
            assert list(status) == [0] * (n - 1) + [3], "the corrupted proof was not the only failure"
        rows.append(dict(n=n, min_ms=1e3 * min(times), proofs_per_s=n / min(times)))
    vk.close()
    return dict(step="gpu", curve="bls12-381", nb_public=nb_public, key_ms=t_key, first_batch_ms=t_first, rows=rows)


def step_endo(reps):
    """the endomorphism checks against the multiplication by r, 16384 valid points"""
    import random
    import bls12_381_oracle as bo
    from gnark_amd import msm
    from gnark_amd._lib import check, lib, ptr
    n = 16384
    rng = random.Random(13)
    ks = bo.fr_vec_to_bytes([rng.randrange(1, bo.R) for _ in range(n)])
    pts = {"g1": bytes(msm.batch_scalar_mul(msm.BLS12_381_G1, bo.g1_to_bytes(bo.G1_GEN), ks, n)),
           "g2": bytes(msm.batch_scalar_mul(msm.BLS12_381_G2, bo.g2_to_bytes(bo.G2_GEN), ks, n))}
    rows = []
    for g in ("g1", "g2"):
        ms = {}
        for kind, name in (("plain", "gg_%s_check_bls12_381" % g), ("endo", "gg_%s_check_endo_bls12_381" % g)):
            fn, flags, times = getattr(lib, name), bytearray(n), []
            for it in range(reps + 1):
                t0 = time.perf_counter()
                check(fn(n, ptr(pts[g]), ptr(flags)))
                dt = time.perf_counter() - t0
                assert not any(flags), "%s rejected a valid point" % name
                if it:
                    times.append(dt)
            ms[kind] = 1e3 * min(times)
        rows.append(dict(group=g, n=n, plain_ms=ms["plain"], endo_ms=ms["endo"], ratio=ms["plain"] / ms["endo"]))
    return dict(step="endo", rows=rows)


def step_oracle(nb_public):
    import bn254_oracle as o
    key, proofs, wits = _instances(nb_public)
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert o.verify(proofs[0], key.vk, wits[0])
        t.append(time.perf_counter() - t0)
    return dict(step="oracle", nb_public=nb_public, seconds=min(t))


def step_resources(source="groth16_verify.hip"):
    src = os.path.join(ROOT, "gnark-fork_amd", "csrc", source)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-munsafe-fp-atomics",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", os.devnull, src]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, check=True).stderr
    kernels, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            name = re.search(r"(k_[a-z0-9_]+?)(?:E[mPN]|I)", v)
            cur = dict(name=name.group(1) if name else v)
            kernels.append(cur)
        elif cur is not None:
            cur[k.split(" ")[0]] = int(v)
    return dict(step="resources", kernels=kernels)


def _child(step, nb_public, sizes, reps, limit, curve="bn254"):
    js = os.path.join(ROOT, "profiles", ".bench_verify_%s_%d.json" % (step, nb_public))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
           "--curve", curve, "--nb-public", str(nb_public), "--reps", str(reps), "--json", js,
           "--n"] + [str(n) for n in sizes]
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:  # nothing more on the GPU after a failed step
        sys.exit("step %s (nb_public %d) ended with status %d" % (step, nb_public, rc))
    res = json.load(open(js))
    os.remove(js)
    return res


def report_bls(a):
    """--curve bls12-381 / both: the BLS12-381 verifier (beside the BN254 one), the endomorphism gate"""
    runs = [_child("gpu", nbp, a.n, a.reps, 400, a.curve) for nbp in a.nb_public]
    endo = _child("endo", 0, a.n, a.reps, 240, a.curve)
    res = json.load(open(a.resources_json)) if a.resources_json else step_resources("groth16_verify_bls.hip")
    out = ["# Groth16 Verify over BLS12-381 on the GPU (tools/bench_verify.py --curve %s)" % a.curve, "",
           "Synthetic instances, one MI355X; gg_groth16_verify_batch_bls12_381 on packed host buffers (uploads and the",
           "status read-back included), min of %d calls after a warm-up; per key shape every size and both curves" % a.reps,
           "run in one process.  Every proof gets its own deterministic verdict.", ""]
    for r in runs:
        bls, bn = r["bls12-381"], r.get("bn254")
        out += ["nb_public = %d:" % bls["nb_public"], "",
                "| proofs per call | BLS12-381 ms | BLS12-381 proofs/s |" + (" BN254 ms | BN254 proofs/s | BLS / BN |" if bn else ""),
                "|---|---|---|" + ("---|---|---|" if bn else "")]
        for i, n in enumerate(a.n):
            row = "| %d | %.2f | %.0f |" % (n, bls["rows"][i]["min_ms"], bls["rows"][i]["proofs_per_s"])
            if bn:
                row += " %.2f | %.0f | %.2f |" % (bn["rows"][i]["min_ms"], bn["rows"][i]["proofs_per_s"],
                                                  bls["rows"][i]["min_ms"] / bn["rows"][i]["min_ms"])
            out.append(row)
        out += ["", "Key creation on the host (line tables, e(alpha, beta)^3): %.1f ms; the first device batch (upload, "
                "the window table of K[1:], one proof): %.1f ms." % (bls["key_ms"], bls["first_batch_ms"]) +
                (" BN254 key creation: %.1f ms." % bn["key_ms"] if bn else ""), ""]
    out += ["Membership checks, %d valid points, host buffers in, flags out, min of %d calls after a warm-up:" %
            (endo["rows"][0]["n"], a.reps), "",
            "| group | multiplication by r, ms | endomorphism check, ms | ratio |", "|---|---|---|---|"]
    for r in endo["rows"]:
        out.append("| %s | %.2f | %.2f | %.2f |" % (r["group"].upper(), r["plain_ms"], r["endo_ms"], r["ratio"]))
    out += ["", "Code objects (gfx950, the compiler's resource remarks):", "",
            "| kernel | VGPRs | SGPRs | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|"]
    for k in res["kernels"]:
        out.append("| %s | %d | %d | %d | %d | %d |" % (k["name"], k.get("VGPRs", 0), k.get("TotalSGPRs", 0),
                                                       k.get("ScratchSize", 0), k.get("LDS", 0), k.get("Occupancy", 0)))
    text = "\n".join(out) + "\n"
    with open(a.out or os.path.join(ROOT, "profiles", "r13_bls12_381_groth16_verify.md"), "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", choices=["bn254", "bls12-381", "both"], default="bn254")
    ap.add_argument("--n", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--nb-public", type=int, nargs="+", default=[2, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="default: profiles/r10_groth16_verify.md, r13_bls12_381_groth16_verify.md "
                                  "with --curve bls12-381 / both")
    ap.add_argument("--resources-json")
    ap.add_argument("--step", choices=["gpu", "oracle", "resources", "endo"])
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step:  # a child: one step
        if a.step == "gpu" and a.curve != "bn254":   # both curves in one process, BN254 first
            res = {"bn254": step_gpu(a.nb_public[0], a.n, a.reps)} if a.curve == "both" else {}
            res["bls12-381"] = step_gpu_bls(a.nb_public[0], a.n, a.reps)
        else:
            res = (step_gpu(a.nb_public[0], a.n, a.reps) if a.step == "gpu" else
                   step_endo(a.reps) if a.step == "endo" else
                   step_oracle(a.nb_public[0]) if a.step == "oracle" else step_resources())
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    if a.curve != "bn254":
        return report_bls(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "r10_groth16_verify.md")
    gpu = [_child("gpu", nbp, a.n, a.reps, 240) for nbp in a.nb_public]
    orc = [_child("oracle", nbp, a.n, a.reps, 120) for nbp in a.nb_public]
    res = json.load(open(a.resources_json)) if a.resources_json else step_resources()
    out = ["# Groth16 Verify on the GPU (tools/bench_verify.py)", "",
           "BN254, synthetic instances, one MI355X; gg_groth16_verify_batch on packed host buffers (uploads and the",
           "status read-back included), min of %d calls after a warm-up, every size in one process per key shape." % a.reps,
           "Every proof gets its own deterministic verdict (no random linear combination).", "",
           "| proofs per call | " + " | ".join("nb_public = %d: ms / proofs per s" % g["nb_public"] for g in gpu) + " |",
           "|---|" + "---|" * len(gpu)]
    for i, n in enumerate(a.n):
        out.append("| %d | " % n + " | ".join("%.2f / %.0f" % (g["rows"][i]["min_ms"], g["rows"][i]["proofs_per_s"])
                                              for g in gpu) + " |")
    out += ["", "Key creation (upload, line tables, e(alpha, beta)^m, the window table of K[1:]): " +
            ", ".join("%.1f ms at nb_public = %d" % (g["key_ms"], g["nb_public"]) for g in gpu) + ".",
            "Baseline, oracle/bn254_oracle.py:verify for one proof on the host CPU: " +
            ", ".join("%.2f s at nb_public = %d" % (r["seconds"], r["nb_public"]) for r in orc) + ".", "",
            "Code objects (gfx950, the compiler's resource remarks):", "",
            "| kernel | VGPRs | SGPRs | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|"]
    for k in res["kernels"]:
        out.append("| %s | %d | %d | %d | %d | %d |" % (k["name"], k.get("VGPRs", 0), k.get("TotalSGPRs", 0),
                                                       k.get("ScratchSize", 0), k.get("LDS", 0), k.get("Occupancy", 0)))
    text = "\n".join(out) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

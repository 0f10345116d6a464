"""PlonK Verify on the GPU: proofs per second for batches under one key.

    python tools/bench_plonk_verify.py [--n 1 64 1024 16384] [--shape 2,0 64,1] [--reps 3]
                                       [--curve bn254|bls12-381|both]
                                       [--resources-json FILE] [--out profiles/r11_plonk_verify.md]

--curve bn254 (the default) is the BN254 report described below.  bls12-381 and
both measure gg_plonk_verify_batch_bls12_381 the same way; with both, the two
curves of a shape run in one child process, sizes interleaved, and the report
(default profiles/r14_bls12_381_plonk_verify_bench.md) gives the BLS12-381 /
BN254 ratio of the call times beside the phase split of either curve, and the
resource figures of both translation units.

BN254 circuits of 2^8 rows (tests/plonk_circuits.py) with (nb_public, n_cmt)
public inputs and BSB22 commitments; 16 distinct proofs made by the GPU prover,
tiled to the batch size.  The driver starts every measured step as a fresh
child process under its own `timeout` and stops at the first one that fails:
  gpu        gnark_amd gg_plonk_verify_batch on packed host buffers (uploads,
             both host hashing steps and the status read-back included), one
             warm-up call per size and then --reps timed ones, the min
             reported; every status must be OK, and one corrupted proof per
             batch must be the only failure.  One more call per size with the
             library's profile on splits the time into the device phases
             (events around each) and the host's share (the rest);
  groth16    gg_groth16_verify_batch at the same batch sizes (tools/bench_verify.py);
  ref        tests/plonk_verify_ref.py:verify for one proof on this CPU;
  resources  the code-object figures of plonk_verify.hip's kernels from the
             compiler's resource remarks; needs no GPU (--step resources --json
             FILE writes them, --resources-json FILE reuses them)."""
import argparse
import ctypes
import json
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnark-fork_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

DISTINCT = 16
LOG_N = 8
TAU = 0x5eed0123456789abcdef


def _curve_mods(curve):
    """(oracle, reference, key class, fr Montgomery encoder, batch entry point) of a curve"""
    from gnark_amd import fr, plonk_verify as pv
    from gnark_amd._lib import lib
    if curve == "bls12-381":
        import bls12_381_oracle as o
        import bls_plonk_verify_ref as ref
        return o, ref, pv.Bls12381VerifyingKey, fr.bls_fr_mont, lib.gg_plonk_verify_batch_bls12_381
    import bn254_oracle as o
    import plonk_verify_ref as ref
    return o, ref, pv.VerifyingKey, fr.fr_mont, lib.gg_plonk_verify_batch


def _instances(nb_public, n_cmt, curve="bn254"):
    """(proving key, verifying key, proofs, witnesses) made on the GPU"""
    from plonk_circuits import Circuit, make_key
    from gnark_amd import plonk_prover as pp
    o, ref, key_cls, _, _ = _curve_mods(curve)
    circ = Circuit(LOG_N, 500 + nb_public, nb_public=nb_public, n_cmt=n_cmt, curve=curve)
    pk = make_key(circ, TAU)
    proofs, wits = [], []
    for i in range(DISTINCT):
        L, Rv, O, pub, cmts = circ.solve(pk, 50 + i, commit=pk.commit_lagrange)
        proofs.append(pp.prove(pk, L, Rv, O, rng=random.Random(i), public=pub, commitments=cmts))
        wits.append(list(pub))
    t0 = time.perf_counter()
    vk = key_cls(pk.vk, o.g1_to_bytes(o.G1_GEN), ref.g2_bytes(TAU))
    return pk, vk, proofs, wits, 1e3 * (time.perf_counter() - t0)


def _profile(name):
    from gnark_amd._lib import check, lib
    ms, k, u = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    check(lib.gg_profile_get(name.encode(), ctypes.byref(ms), ctypes.byref(k), ctypes.byref(u)))
    return ms.value


class _Bench:
    """one curve's key, packed proofs and timed call"""

    def __init__(self, nb_public, n_cmt, curve):
        from gnark_amd import plonk_prover as pp
        from gnark_amd._lib import HASH_FN
        o, _, _, mont, self.fn = _curve_mods(curve)
        self.curve = curve
        self.pk, self.vk, proofs, wits, self.t_key = _instances(nb_public, n_cmt, curve)
        self.pb = [pp.proof_bytes(p, curve) for p in proofs]
        self.wb = [b"".join(mont(x) for x in w) for w in wits]
        self.size = size = len(self.pb[0])
        pt = 96 if curve == "bls12-381" else 64
        self.bad = bytearray(self.pb[0])  # ZShiftedOpening.H + G: the second opening alone fails
        self.bad[size - pt - 32:size - 32] = o.g1_to_bytes(o.g1_add(o.g1_from_bytes(proofs[0].z_shifted_H), o.G1_GEN))
        self.none = HASH_FN()
        self.rows = []

    def call(self, packed, wit, status, n):
        from gnark_amd._lib import check, ptr
        t0 = time.perf_counter()
        check(self.fn(self.vk.handle, n, ptr(packed), ptr(wit) if wit else None, self.none, None, self.none, None,
                      ptr(status)))
        return time.perf_counter() - t0

    def measure(self, n, reps):
        from gnark_amd._lib import check, lib
        packed = bytearray(b"".join(self.pb[i % DISTINCT] for i in range(n)))
        wit = b"".join(self.wb[i % DISTINCT] for i in range(n))
        status = bytearray(n)
        times = []
        for it in range(reps + 1):  # the first call warms up (code objects, the key's buffers)
            dt = self.call(packed, wit, status, n)
            assert not any(status), "a valid proof was rejected at n = %d" % n
            if it:
                times.append(dt)
        check(lib.gg_profile_enable(1))
        wall = self.call(packed, wit, status, n)
        p1, p2 = _profile("plonk_verify_phase1"), _profile("plonk_verify_phase2")
        check(lib.gg_profile_enable(0))
        if (n - 1) % DISTINCT == 0:
            packed[self.size * (n - 1):self.size * n] = self.bad
            self.call(packed, wit, status, n)
            assert list(status) == [0] * (n - 1) + [3], "the corrupted proof was not the only failure"
        self.rows.append(dict(n=n, min_ms=1e3 * min(times), proofs_per_s=n / min(times), phase1_ms=p1, phase2_ms=p2,
                              host_ms=1e3 * wall - p1 - p2))

    def close(self):
        self.vk.close()
        self.pk.close()


def step_gpu(nb_public, n_cmt, sizes, reps, curve="bn254"):
    curves = ["bls12-381", "bn254"] if curve == "both" else [curve]
    benches = [_Bench(nb_public, n_cmt, c) for c in curves]
    for n in sizes:  # the curves of one size next to each other: a ratio of like conditions
        for b in benches:
            b.measure(n, reps)
    for b in benches:
        b.close()
    first = benches[0]
    return dict(step="gpu", nb_public=nb_public, n_cmt=n_cmt, key_ms=first.t_key, rows=first.rows, curve=first.curve,
                others=[dict(curve=b.curve, key_ms=b.t_key, rows=b.rows) for b in benches[1:]])


def step_ref(nb_public, n_cmt, curve="bn254"):
    ref = _curve_mods(curve)[1]
    pk, vk, proofs, wits, _ = _instances(nb_public, n_cmt, curve)
    kd, g2, op = ref.key_dict_from_lib(pk.vk), ref.g2_pair(TAU), ref.oracle_proof(proofs[0])
    t = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert ref.verify(kd, g2, op, wits[0]) == ref.OK
        t.append(time.perf_counter() - t0)
    vk.close()
    pk.close()
    return dict(step="ref", nb_public=nb_public, n_cmt=n_cmt, seconds=min(t))


def step_groth16(nb_public, sizes, reps):
    import bench_verify
    return bench_verify.step_gpu(nb_public, sizes, reps)


def step_resources(curve="bn254"):
    if curve == "both":
        return dict(step="resources", kernels=step_resources("bls12-381")["kernels"] +
                    step_resources("bn254")["kernels"])
    src = os.path.join(ROOT, "gnark-fork_amd", "csrc",
                       "plonk_verify_bls.hip" if curve == "bls12-381" else "plonk_verify.hip")
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
            name = re.search(r"(k_[a-z0-9_]+?)E", v)
            cur = dict(name=name.group(1) if name else v)
            kernels.append(cur)
        elif cur is not None:
            cur[k.split(" ")[0]] = int(v)
    return dict(step="resources", kernels=kernels)


def _child(step, shape, sizes, reps, limit, curve="bn254"):
    js = os.path.join(ROOT, "profiles", ".bench_plonk_verify_%s_%d_%d.json" % (step, shape[0], shape[1]))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
           "--shape", "%d,%d" % shape, "--reps", str(reps), "--curve", curve, "--json", js, "--n"] + [str(n) for n in sizes]
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:  # nothing more on the GPU after a failed step
        sys.exit("step %s (shape %s) ended with status %d" % (step, shape, rc))
    res = json.load(open(js))
    os.remove(js)
    return res


RESOURCE_HEAD = ["| kernel | VGPRs | SGPRs | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|"]


def resource_rows(res):
    return ["| %s | %d | %d | %d | %d | %d |" % (k["name"], k.get("VGPRs", 0), k.get("TotalSGPRs", 0),
                                                 k.get("ScratchSize", 0), k.get("LDS", 0), k.get("Occupancy", 0))
            for k in res["kernels"]]


def report_bls(a, shapes):
    """--curve bls12-381 / both: the BLS12-381 call times and phase split, beside BN254's with both"""
    out_path = a.out or os.path.join(ROOT, "profiles", "r14_bls12_381_plonk_verify_bench.md")
    gpu = [_child("gpu", s, a.n, a.reps, 600, a.curve) for s in shapes]
    refs = [_child("ref", s, a.n, a.reps, 240, "bls12-381") for s in shapes]
    res = json.load(open(a.resources_json)) if a.resources_json else step_resources(a.curve)
    out = ["# PlonK Verify over BLS12-381 on the GPU (tools/bench_plonk_verify.py --curve %s)" % a.curve, "",
           "Circuits of 2^%d rows, %d distinct proofs made by the GPU prover and tiled to the batch size, one MI355X;" %
           (LOG_N, DISTINCT),
           "gg_plonk_verify_batch_bls12_381 on packed host buffers (uploads, both host hashing steps and the status",
           "read-back included), min of %d calls after a warm-up; per shape every size and both curves run in one" %
           a.reps, "process.  p1 / p2 / host: one more call with the library's profile on (device phase 1, device",
           "phase 2, the rest of the call).", ""]
    for g in gpu:
        out += ["## nb_public = %d, n_cmt = %d" % (g["nb_public"], g["n_cmt"]), ""]
        bn = g["others"][0]["rows"] if g["others"] else None
        head = "| proofs per call | BLS12-381 ms | proofs per s | p1 ms | p2 ms | host ms |"
        if bn:
            head += " BN254 ms | proofs per s | p1 ms | p2 ms | host ms | BLS / BN |"
        out += [head, "|" + "---|" * (head.count("|") - 1)]
        for i, r in enumerate(g["rows"]):
            row = "| %d | %.2f | %.0f | %.2f | %.2f | %.2f |" % (r["n"], r["min_ms"], r["proofs_per_s"], r["phase1_ms"],
                                                                r["phase2_ms"], r["host_ms"])
            if bn:
                q = bn[i]
                row += " %.2f | %.0f | %.2f | %.2f | %.2f | %.2f |" % (q["min_ms"], q["proofs_per_s"], q["phase1_ms"],
                                                                      q["phase2_ms"], q["host_ms"],
                                                                      r["min_ms"] / q["min_ms"])
            out.append(row)
        out.append("")
    out += ["Key creation on the host (validation with the subgroup tests, the two line tables): " +
            ", ".join("%.1f ms at (%d, %d)" % (g["key_ms"], g["nb_public"], g["n_cmt"]) for g in gpu) + ".",
            "Baseline, tests/bls_plonk_verify_ref.py:verify for one proof on the host CPU: " +
            ", ".join("%.2f s at (%d, %d)" % (r["seconds"], r["nb_public"], r["n_cmt"]) for r in refs) + ".", "",
            "Code objects (gfx950, the compiler's resource remarks):", ""] + RESOURCE_HEAD + resource_rows(res)
    text = "\n".join(out) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--shape", nargs="+", default=["2,0", "64,1"], help="nb_public,n_cmt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--curve", choices=["bn254", "bls12-381", "both"], default="bn254")
    ap.add_argument("--out")
    ap.add_argument("--resources-json")
    ap.add_argument("--step", choices=["gpu", "groth16", "ref", "resources"])
    ap.add_argument("--json")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape]
    if a.step:  # a child: one step
        s = shapes[0]
        res = (step_gpu(s[0], s[1], a.n, a.reps, a.curve) if a.step == "gpu" else
               step_groth16(s[0], a.n, a.reps) if a.step == "groth16" else
               step_ref(s[0], s[1], a.curve) if a.step == "ref" else step_resources(a.curve))
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    if a.curve != "bn254":
        return report_bls(a, shapes)
    a.out = a.out or os.path.join(ROOT, "profiles", "r11_plonk_verify.md")
    gpu = [_child("gpu", s, a.n, a.reps, 300) for s in shapes]
    g16 = [_child("groth16", (max(s[0], 1), 0), a.n, a.reps, 240) for s in shapes]
    refs = [_child("ref", s, a.n, a.reps, 180) for s in shapes]
    res = json.load(open(a.resources_json)) if a.resources_json else step_resources()
    out = ["# PlonK Verify on the GPU (tools/bench_plonk_verify.py)", "",
           "BN254, circuits of 2^%d rows, %d distinct proofs made by the GPU prover and tiled to the batch size, one" %
           (LOG_N, DISTINCT),
           "MI355X; gg_plonk_verify_batch on packed host buffers (uploads, both host hashing steps and the status",
           "read-back included), min of %d calls after a warm-up.  Every proof gets its own deterministic verdict." %
           a.reps, ""]
    for g, q in zip(gpu, g16):
        out += ["## nb_public = %d, n_cmt = %d" % (g["nb_public"], g["n_cmt"]), "",
                "| proofs per call | ms | proofs per s | device phase 1 ms | device phase 2 ms | host ms |"
                " Groth16 Verify (nb_public = %d) ms / proofs per s |" % q["nb_public"], "|---|---|---|---|---|---|---|"]
        for r, r16 in zip(g["rows"], q["rows"]):
            out.append("| %d | %.2f | %.0f | %.2f | %.2f | %.2f | %.2f / %.0f |" %
                       (r["n"], r["min_ms"], r["proofs_per_s"], r["phase1_ms"], r["phase2_ms"], r["host_ms"],
                        r16["min_ms"], r16["proofs_per_s"]))
        out.append("")
    out += ["The split is one more call with the library's profile on: phase 1 = uploads, PI(zeta), the quotient",
            "identity, foldedH and the linearised digest, read-back; phase 2 = uploads, A and B, the pairing check,",
            "read-back; host = the rest of that call (transcripts, BSB22 hashes, the KZG folding challenge, lambda).", "",
            "Key creation (validation, the two line tables, on the host): " +
            ", ".join("%.1f ms at (%d, %d)" % (g["key_ms"], g["nb_public"], g["n_cmt"]) for g in gpu) + ".",
            "Baseline, tests/plonk_verify_ref.py:verify for one proof on the host CPU: " +
            ", ".join("%.2f s at (%d, %d)" % (r["seconds"], r["nb_public"], r["n_cmt"]) for r in refs) + ".", "",
            "Code objects (gfx950, the compiler's resource remarks):", ""] + RESOURCE_HEAD + resource_rows(res)
    text = "\n".join(out) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

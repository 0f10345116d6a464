"""C-ABI checks that need no GPU: the library loads, every symbol declared in
include/gnark_amd.h is exported, host-side helpers are exact, errors surface."""
import ctypes
import os
import re

import pytest

import bn254_oracle as o
from helpers import b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    import gnark_amd
    lib = ctypes.CDLL(gnark_amd.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    # and the Python binding declares every one of them
    from gnark_amd import _lib
    assert sorted(_lib.EXPORTED) == syms


def test_version_and_errors():
    import gnark_amd
    from gnark_amd import _lib
    assert _lib.lib.gg_version() >= 100
    h = ctypes.c_void_p()
    bad_omega = o.fr_to_bytes(2)  # not a root of unity of order 8
    rc = _lib.lib.gg_domain_create(3, _lib.ptr(bad_omega), _lib.ptr(o.fr_to_bytes(5)), ctypes.byref(h))
    assert rc == 1  # GG_ERR_INVALID_ARG
    assert b"omega" in _lib.lib.gg_last_error()
    with pytest.raises(gnark_amd.GnarkAmdError):
        gnark_amd.ntt.Domain(3, omega_mont=bad_omega)


def test_host_point_helpers_match_oracle():
    from gnark_amd import msm
    rng = o.SplitMix64(99)
    for _ in range(3):
        k1, k2, s = rng.fr(), rng.fr(), rng.fr()
        p1, p2 = o.g1_mul(o.G1_GEN, k1), o.g1_mul(o.G1_GEN, k2)
        j = msm.scalar_mul(msm.G1, o.g1_to_bytes(p1), o.fr_to_bytes(s))
        assert o.g1_from_bytes(msm.jac_to_affine(msm.G1, j)) == o.g1_mul(p1, s)
        j2 = msm.scalar_mul(msm.G1, o.g1_to_bytes(p2), o.fr_to_bytes(1))
        tot = msm.jac_add(msm.G1, j, j2)
        assert o.g1_from_bytes(msm.jac_to_affine(msm.G1, tot)) == o.g1_add(o.g1_mul(p1, s), p2)
        q = o.g2_mul(o.G2_GEN, k1)
        j = msm.scalar_mul(msm.G2, o.g2_to_bytes(q), o.fr_to_bytes(s))
        assert o.g2_from_bytes(msm.jac_to_affine(msm.G2, j)) == o.g2_mul(q, s)
    # P + (-P) = infinity, P + P = 2P
    p = o.g1_mul(o.G1_GEN, 77)
    jp = msm.scalar_mul(msm.G1, o.g1_to_bytes(p), o.fr_to_bytes(1))
    jn = msm.scalar_mul(msm.G1, o.g1_to_bytes(p), o.fr_to_bytes(o.R - 1))
    assert msm.jac_to_affine(msm.G1, msm.jac_add(msm.G1, jp, jn)) == bytes(64)
    assert o.g1_from_bytes(msm.jac_to_affine(msm.G1, msm.jac_add(msm.G1, jp, jp))) == o.g1_mul(p, 2)


def test_backend_options_mirror():
    from gnark_amd import backend
    cfg = backend.new_prover_config()
    assert not backend.accelerated(cfg)
    cfg = backend.new_prover_config(backend.with_icicle_acceleration())
    assert backend.accelerated(cfg) and cfg.accelerator == "amd"


def test_proof_raw_encoding_matches_oracle():
    from helpers import golden
    from gnark_amd import groth16
    g = golden()["groth16"][0]
    pr = groth16.Proof(b(g["Ar"]), b(g["Bs"]), b(g["Krs"]))
    assert pr.write_raw()[:256].hex() == g["raw_prefix"]


def test_multi_gpu_timing_and_rehearsal_abi():
    """The N-GPU instrumentation and rehearsal entry points (no GPU needed: the
    argument checks run first): slot counts agree between header and binding,
    null handles / short buffers / bad shards are GG_ERR_INVALID_ARG, and
    GG_REHEARSAL is distinct from every error code."""
    from gnark_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    consts = dict(re.findall(r"#define (GG_[A-Z0-9_]+) ([0-9]+)\b", src))
    assert int(consts["GG_REHEARSAL"]) == _lib.GG_REHEARSAL == 7
    assert int(consts["GG_PLONK_PART_SLOTS"]) == _lib.GG_PLONK_PART_SLOTS
    assert 2 + 4 * int(consts["GG_MPK_MAX_EXCHANGES"]) == _lib.GG_MPK_TIMING_SLOTS
    errs = {int(v) for k, v in consts.items() if k.startswith("GG_ERR_")}
    assert _lib.GG_REHEARSAL not in errs and _lib.GG_REHEARSAL != _lib.GG_OK
    buf = (ctypes.c_double * 32)()
    L = _lib.lib
    assert L.gg_groth16_mpk_shard_timings(None, 0, buf, 32) == 1
    assert L.gg_groth16_mpk_set_rehearsal(None, 0) == 1
    assert L.gg_plonk_pk_part_timings(None, 0, buf, 32) == 1
    assert L.gg_plonk_pk_set_rehearsal(None, 1) == 1
    assert L.gg_hshard_exchange_bytes(None, 1, ctypes.byref(ctypes.c_size_t())) == 1
    assert b"null" in L.gg_last_error()


def test_peer_access_and_build_flags_abi():
    """Round 5 diagnostics of a first N-GPU run: the GG_PEER_* codes agree
    between header and binding, the peer-access queries check their arguments,
    and the product library is not a diagnostic (probe) build."""
    from gnark_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    consts = dict(re.findall(r"#define (GG_[A-Z0-9_]+) ([0-9]+)\b", src))
    peer = {int(v): k for k, v in consts.items() if k.startswith("GG_PEER_")}
    assert sorted(peer) == sorted(_lib.PEER_ACCESS) == [0, 1, 2, 3]
    assert peer[0] == "GG_PEER_SAME_DEVICE" and peer[1] == "GG_PEER_ENABLED"
    assert int(consts["GG_BUILD_ACCUM_PROBE"]) == _lib.GG_BUILD_ACCUM_PROBE
    assert _lib.lib.gg_build_flags() == _lib.BUILD_FLAGS == 0
    codes = (ctypes.c_int * 64)()
    k = ctypes.c_int()
    assert _lib.lib.gg_groth16_mpk_peer_access(None, codes, 64) == 1
    assert _lib.lib.gg_plonk_pk_peer_access(None, codes, 64, ctypes.byref(k)) == 1


def test_bench_reports_planned_exchange_and_devices():
    """bench.py's N-GPU fields (round-4 VERDICT Weak 6): the split projection
    reports the planned all-to-all bytes (not the rehearsal's zero pushes), torch
    mode counts distinct devices and refuses a shared GPU under RCCL, and the
    collective is named after the backend."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "exchange_bytes_after" in src and '"exchange_MB_per_shard"' in src
    assert "len(set(rank_devices))" in src and "distinct GPU(s)" in src
    assert '"RCCL" if backend == "nccl" else backend' in src
    assert "1/%d slice per GPU" not in src


def test_bench_dump_outputs_round_trips(tmp_path):
    """bench.py --dump-outputs: one float64 .npy per proof point, each byte kept
    exactly (no GPU needed: the writer only takes a Proof)."""
    import numpy as np
    import bench
    from helpers import golden
    from gnark_amd import groth16
    g = golden()["groth16"][0]
    pr = groth16.Proof(b(g["Ar"]), b(g["Bs"]), b(g["Krs"]))
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), pr)
    assert sorted(p.name for p in out.iterdir()) == ["Ar.npy", "Bs.npy", "Krs.npy"]
    for name, size in (("Ar", 64), ("Bs", 128), ("Krs", 64)):
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == (size,)
        assert a.astype(np.uint8).tobytes() == getattr(pr, name)


def test_bench_plain_run_is_the_headline_only():
    """bench.py: the extra measurements sit behind --full (off by default), and
    --dump-outputs takes a directory."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_every_environment_knob_is_documented():
    """Every GG_* variable the library reads is in INTEGRATION.md's tables."""
    csrc = os.path.join(ROOT, "gnark-fork_amd", "csrc")
    knobs = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cuh", ".h")):
            with open(os.path.join(csrc, f)) as fh:
                knobs.update(re.findall(r'getenv\("(GG_[A-Z0-9_]+)"\)', fh.read()))
    assert "GG_TASK_QUEUES" in knobs
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    missing = sorted(k for k in knobs if f"`{k}`" not in doc)
    assert not missing, missing


def test_bounded_wait_times_out_instead_of_blocking():
    """A barrier of 3 parts that only 2 reach: both waiters return GG_ERR_TIMEOUT
    after the deadline (host only, no GPU) and the message names the wait --
    the library's part barriers and stream / event waits share this deadline
    (gg_set_wait_timeout; VERDICT r5: a stall must end in an error)."""
    import time
    from gnark_amd import _lib
    t = time.time()
    rc = _lib.lib.gg_wait_selftest(3, 2, 0.5)
    el = time.time() - t
    assert rc == _lib.GG_ERR_TIMEOUT
    msg = _lib.lib.gg_last_error().decode()
    assert "timed out" in msg and "barrier of 3 (2 arrived)" in msg and "selftest part" in msg
    assert 0.4 < el < 10
    assert _lib.lib.gg_wait_selftest(3, 3, 0.5) == 0  # everyone arrives: no timeout
    # the process-wide deadline is settable and restored
    assert _lib.lib.gg_set_wait_timeout(12.5) == 0 and _lib.lib.gg_get_wait_timeout() == 12.5
    assert _lib.lib.gg_set_wait_timeout(0) == 0 and _lib.lib.gg_get_wait_timeout() > 0
    assert _lib.lib.gg_set_wait_timeout(-1) == 1
    # the real-stream variant (tests/test_gpu_wait_timeout.py) checks its
    # arguments before touching the device
    assert _lib.lib.gg_wait_selftest_device(10, 0.0) == 1
    assert _lib.lib.gg_wait_selftest_device((1 << 20) + 1, 1.0) == 1


def test_kept_worker_threads_run_blocked_tasks_and_return_errors():
    """The provers' host tasks run on kept worker threads (common.h run_task,
    round 6): 64 tasks that all wait at one barrier need 64 workers at once --
    the set grows instead of deadlocking -- and the failing task's error comes
    back to the waiter, as with std::async (host only, no GPU)."""
    from gnark_amd import _lib
    for n in (1, 8, 64):
        assert _lib.lib.gg_task_selftest(n) == 0, _lib.lib.gg_last_error()
    assert _lib.lib.gg_task_selftest(0) == 1
    # the A/B switch (a fresh thread per task) keeps the same contract; the
    # variable is read once per process, hence a child process
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from gnark_amd import _lib; "
            "rc = _lib.lib.gg_task_selftest(16); print(rc, _lib.lib.gg_last_error().decode()); "
            "sys.exit(rc)" % os.path.join(ROOT, "gnark-fork_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GG_TASK_POOL="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_msm_batch_shape_refuses_32bit_overflow():
    """a batch multiplies the sort's entries by n_vectors and its
    bucket space by the next power of two; past 32-bit words it is refused
    (GG_ERR_UNSUPPORTED), and the PlonK prover then commits one MSM per vector."""
    from gnark_amd import _lib
    L = _lib.lib
    # PlonK 2^22 on BLS12-381: c = 20, W = 13 windows -- fits for 3 and 4 vectors
    assert L.gg_msm_batch_shape(1 << 22, 20, 13, 1, 3) == 0
    assert L.gg_msm_batch_shape(1 << 22, 20, 13, 1, 4) == 0
    # 2^27 points x 11 windows x 3 vectors > 2^32 entries
    assert L.gg_msm_batch_shape(1 << 27, 23, 11, 1, 3) == _lib.GG_ERR_UNSUPPORTED
    assert "2^32" in L.gg_last_error().decode()
    assert L.gg_msm_batch_shape(1 << 27, 23, 11, 1, 1) == 0
    # bucket ids: 4 groups x 2^29 buckets x kp 4 >= 2^31
    assert L.gg_msm_batch_shape(1 << 10, 30, 1, 4, 3) == _lib.GG_ERR_UNSUPPORTED
    assert L.gg_msm_batch_shape(1 << 10, 30, 1, 4, 5) == 1  # n_vectors out of range

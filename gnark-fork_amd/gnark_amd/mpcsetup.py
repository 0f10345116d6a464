"""Groth16 keys from a powers-of-tau SRS: phase 2 of gnark's MPC setup
(backend/groth16/bn254/mpcsetup: InitPhase2, Contribute, ExtractKeys) over the
C ABI's gg_groth16_setup_from_srs / gg_groth16_setup_contribute
(csrc/groth16_mpc_setup.hip).

    srs = Phase1Srs(...)                       # a ceremony's phase-1 parameters
    p2 = init_phase2(nb_public, n_wires, term_off, term_wire, term_coeff, coeffs, srs)
    p2.contribute()                            # once per participant
    pk, vk = p2.extract_keys()                 # groth16.ProvingKeyData / VerifyingKeyData

The ceremony's transcript (the contributions' public keys and hashes,
VerifyPhase1 / VerifyPhase2) stays with gnark; circuits with BSB22 commitments
are not representable, as in the reference."""
from __future__ import annotations

import ctypes
import dataclasses
import secrets
from typing import Optional, Sequence, Union

import numpy as np

from . import fr, groth16, msm
from ._lib import (GG_CURVE_BLS12_381, GG_CURVE_BN254, GG_SETUP_TIMING_SLOTS, DeviceBuffer, check, lib, ptr)

Points = Union[bytes, DeviceBuffer]

TIMINGS = ["transpose", "lagrange", "accumulate", "kz", "g1", "g2", "accumulate_kernels", "accumulate_threads",
           "terms", "ecntt_tau_g1", "ecntt_alpha_tau_g1", "ecntt_beta_tau_g1", "ecntt_tau_g2", "upload_check",
           "general_abc", "accumulate_abc", "general_k", "accumulate_k", "general_g2", "accumulate_g2", "z",
           "normalise", "contribute", "general_terms"]


def _field(curve: str):
    if curve == "bn254":
        return GG_CURVE_BN254, fr.R, fr.fr_mont, fr.domain_generator, msm.G1, msm.G2
    if curve == "bls12-381":
        return GG_CURVE_BLS12_381, fr.BLS_R, fr.bls_fr_mont, fr.bls_domain_generator, msm.BLS12_381_G1, msm.BLS12_381_G2
    raise ValueError("curve must be 'bn254' or 'bls12-381'")


@dataclasses.dataclass
class Phase1Srs:
    """Phase1.Parameters (phase1.go:35-50), affine points in the curve's layout,
    each part as bytes or as a DeviceBuffer: tau_g1 [tau^i]1 (2n - 1 points),
    alpha_tau_g1 [alpha tau^i]1, beta_tau_g1 [beta tau^i]1, tau_g2 [tau^i]2 (n
    points each), beta_g2 [beta]2; n a power of two."""
    tau_g1: Points
    alpha_tau_g1: Points
    beta_tau_g1: Points
    tau_g2: Points
    beta_g2: Points
    n: int
    curve: str = "bn254"


def srs_from_trapdoor(power: int, tau: int, alpha: int, beta: int, curve: str = "bn254") -> Phase1Srs:
    """The SRS of n = 2^power from a KNOWN trapdoor, by msm.batch_scalar_mul of the
    generators.  Single-party and insecure: whoever knows tau, alpha and beta
    forges proofs under every key made from it.  For tests and benchmarks."""
    _, mod, mont, _, g1id, g2id = _field(curve)
    n = 1 << power
    g1, g2 = fr.generators(curve)
    pw = [1] * (2 * n - 1)
    for i in range(1, 2 * n - 1):
        pw[i] = pw[i - 1] * tau % mod
    sc = lambda xs: b"".join(mont(x % mod) for x in xs)
    return Phase1Srs(
        tau_g1=msm.batch_scalar_mul(g1id, g1, sc(pw), 2 * n - 1),
        alpha_tau_g1=msm.batch_scalar_mul(g1id, g1, sc(alpha * x for x in pw[:n]), n),
        beta_tau_g1=msm.batch_scalar_mul(g1id, g1, sc(beta * x for x in pw[:n]), n),
        tau_g2=msm.batch_scalar_mul(g2id, g2, sc(pw[:n]), n),
        beta_g2=msm.batch_scalar_mul(g2id, g2, sc([beta]), 1), n=n, curve=curve)


class Phase2:
    """gg_groth16_setup_from_srs's handle: the key's points in HBM; delta1 / delta2
    start as the generators (phase2.go:142-144)."""

    def __init__(self, handle, curve: str, n_wires: int, nb_public: int):
        self._res = groth16.SetupResult(handle, curve)
        self.curve, self.n_wires, self.nb_public = curve, n_wires, nb_public

    log_n = property(lambda self: self._res.log_n)
    acc_chunk = property(lambda self: self._res.acc_chunk)
    acc_launches = property(lambda self: self._res.acc_launches)

    def contribute(self, delta: Optional[int] = None) -> None:
        """Phase2.Contribute (phase2.go:181-210), the point updates: delta1, delta2
        *= delta; Z, pk.G1.K *= 1/delta.  None samples delta in [1, r) with
        `secrets`; zero is rejected."""
        _, mod, mont, _, _, _ = _field(self.curve)
        if delta is None:
            delta = 1 + secrets.randbelow(mod - 1)
        check(lib.gg_groth16_setup_contribute(self._res.handle, ptr(mont(delta % mod))))

    def extract_keys(self):
        """ExtractKeys (setup.go:25-97) -> (ProvingKeyData, VerifyingKeyData): the
        read-back of groth16.setup.  The handle stays open for further contributions."""
        return groth16.read_keys(self._res, self.n_wires, self.nb_public)

    def timings(self) -> dict:
        """ms per phase and counts (gg_groth16_setup_timings, all slots)"""
        t = (ctypes.c_double * GG_SETUP_TIMING_SLOTS)()
        check(lib.gg_groth16_setup_timings(self._res.handle, t, GG_SETUP_TIMING_SLOTS))
        return dict(zip(TIMINGS, list(t)))

    def close(self):
        self._res.close()


def init_phase2(nb_public: int, n_wires: int, term_off, term_wire, term_coeff, coeffs: Sequence[int],
                srs: Phase1Srs, check_points: bool = True) -> Phase2:
    """InitPhase2 (phase2.go:53-179) on the GPU.  The R1CS as groth16.setup takes
    it; coefficients are classified by value, so any numbering of the table works.
    srs.n may exceed the circuit's domain: the prefixes are used.  check_points
    runs the curve and subgroup checks over what is used; that the SRS is a
    powers-of-tau string at all is the ceremony's VerifyPhase1 to establish."""
    cid, mod, mont, gen, _, _ = _field(srs.curve)
    off = np.ascontiguousarray(term_off, dtype=np.uint32)
    wire = np.ascontiguousarray(term_wire, dtype=np.uint32)
    cidx = np.ascontiguousarray(term_coeff, dtype=np.uint32)
    ncons = (len(off) - 1) // 3
    log_n = max(ncons - 1, 0).bit_length()
    g1, g2 = fr.generators(srs.curve)
    cbytes = b"".join(mont(int(k) % mod) for k in coeffs)
    parts = []
    for p in (srs.tau_g1, srs.alpha_tau_g1, srs.beta_tau_g1, srs.tau_g2, srs.beta_g2):
        dev = isinstance(p, DeviceBuffer)
        parts += [ptr(p if dev else bytes(p)), int(dev)]
    h = ctypes.c_void_p()
    check(lib.gg_groth16_setup_from_srs(
        cid, n_wires, ncons, nb_public, ptr(off), ptr(wire) if len(wire) else None,
        ptr(cidx) if len(cidx) else None, ptr(cbytes), len(coeffs), *parts, srs.n, int(check_points),
        ptr(mont(gen(log_n))), ptr(g1), ptr(g2), ctypes.byref(h)))
    return Phase2(h, srs.curve, n_wires, nb_public)


def init_phase2_from_terms(nb_public: int, n_wires: int, constraints, srs: Phase1Srs, **kw) -> Phase2:
    """init_phase2 for [(L, R, O)] constraint lists (groth16.setup_from_terms' input)."""
    _, mod, *_ = _field(srs.curve)
    off, wires, cids, table = groth16.terms_to_csr(constraints, mod)
    return init_phase2(nb_public, n_wires, off, wires, cids, table, srs, **kw)

"""PlonK Verify (backend/plonk/bn254/verify.go:45-294 and its bls12-381 twin)
for batches of proofs under one verifying key, over the C ABI's
gg_plonk_vk_create / gg_plonk_verify_batch (BN254, csrc/plonk_verify.hip) and
gg_plonk_vk_create_bls12_381 / gg_plonk_verify_batch_bls12_381 (BLS12-381,
csrc/plonk_verify_bls.hip).  The key's class chooses the curve: VerifyingKey
or Bls12381VerifyingKey.

The transcripts (SHA-256 by default, or the caller's hashes) and the BSB22
hashes run on the host inside the library; the point checks, PI(zeta), the
quotient identity, the G1 combinations and the two-pair KZG check
e(A, G2) e(B, [tau]G2) == 1 run on the GPU, or on the calling thread with
host=True.  Every proof gets its own verdict, the same one every time: the
coefficient that joins the two openings is a hash of the proof, not a random
draw."""
from __future__ import annotations

import ctypes
from typing import Callable, Optional, Sequence

import numpy as np

from . import fr, plonk_prover
from ._lib import GG_CURVE_BLS12_381, GG_CURVE_BN254, check, lib, ptr

VERIFY_OK, VERIFY_MALFORMED, VERIFY_QUOTIENT, VERIFY_KZG = 0, 1, 2, 3
_VERIFY_MESSAGES = {
    VERIFY_MALFORMED: "invalid proof: a point is not on the curve (BLS12-381: or not in the subgroup) or a scalar "
                      "is not reduced",
    VERIFY_QUOTIENT: "claimed quotient is not as expected",  # verify.go:42
    VERIFY_KZG: "can't verify opening proof",                # gnark-crypto kzg.ErrVerifyOpeningProof
}


class VerifyError(ValueError):
    """plonk.Verify's error; .status is the GG_PLONK_VERIFY_* value."""

    def __init__(self, status: int):
        super().__init__(_VERIFY_MESSAGES.get(status, f"verify status {status}"))
        self.status = status


class VerifyingKey:
    """The verifying key with its KZG part (gg_plonk_vk_create).  vk: the
    plonk_prover.VerifyingKey of a ProvingKey or of setup(); kzg_g1: the SRS's G1
    generator (64 B affine); kzg_g2: G2 and [tau]G2 (2 x 128 B affine).  The key
    and the two line tables go to the GPU with the first device batch and stay
    there for any number of verify_batch calls."""

    def __init__(self, vk: plonk_prover.VerifyingKey, kzg_g1: bytes, kzg_g2: bytes, curve: str = "bn254"):
        if curve != "bn254":
            raise ValueError("VerifyingKey: curve must be 'bn254' (BLS12-381 keys: Bls12381VerifyingKey)")
        if len(kzg_g1) < 64 or len(kzg_g2) != 256:
            raise ValueError("kzg_g1: one G1Affine (64 bytes); kzg_g2: G2 and [tau]G2 (256 bytes)")
        self.vk = vk
        self.n_commitments, self.nb_public = len(vk.Qcp), vk.nb_public
        idx = np.ascontiguousarray(list(vk.commitment_indexes), dtype=np.uint32)
        h = ctypes.c_void_p()
        nc = self.n_commitments
        check(lib.gg_plonk_vk_create(
            GG_CURVE_BN254, vk.size, ptr(fr.fr_mont(vk.generator)), ptr(fr.fr_mont(vk.coset_shift)),
            ptr(b"".join(vk.S)), ptr(b"".join([vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk])),
            ptr(b"".join(vk.Qcp)) if nc else None, nc, ptr(idx) if nc else None, vk.nb_public,
            ptr(bytes(kzg_g1[:64])), ptr(bytes(kzg_g2)), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            lib.gg_plonk_vk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bls12381VerifyingKey:
    """The verifying key over BLS12-381 (gg_plonk_vk_create_bls12_381).  vk: the
    plonk_prover.VerifyingKey of a BLS12-381 ProvingKey or of setup(); kzg_g1: the
    SRS's G1 generator (96 B affine); kzg_g2: G2 and [tau]G2 (2 x 192 B affine).
    Every G1 point of the key must lie in the order-r subgroup.  Creation runs on
    the host alone; the first device batch uploads the key and its line tables."""
    curve = "bls12-381"

    def __init__(self, vk: plonk_prover.VerifyingKey, kzg_g1: bytes, kzg_g2: bytes):
        if len(kzg_g1) < 96 or len(kzg_g2) != 384:
            raise ValueError("kzg_g1: one G1Affine (96 bytes); kzg_g2: G2 and [tau]G2 (384 bytes)")
        self.vk = vk
        self.n_commitments, self.nb_public = len(vk.Qcp), vk.nb_public
        idx = np.ascontiguousarray(list(vk.commitment_indexes), dtype=np.uint32)
        h = ctypes.c_void_p()
        nc = self.n_commitments
        check(lib.gg_plonk_vk_create_bls12_381(
            vk.size, ptr(fr.bls_fr_mont(vk.generator)), ptr(fr.bls_fr_mont(vk.coset_shift)),
            ptr(b"".join(vk.S)), ptr(b"".join([vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk])),
            ptr(b"".join(vk.Qcp)) if nc else None, nc, ptr(idx) if nc else None, vk.nb_public,
            ptr(bytes(kzg_g1[:96])), ptr(bytes(kzg_g2)), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            lib.gg_plonk_vk_destroy_bls12_381(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_bls(vk) -> bool:
    return isinstance(vk, Bls12381VerifyingKey)


def _witness_bytes(w, bls: bool = False) -> bytes:
    """fr Montgomery bytes of a public witness given as bytes or as integers."""
    if isinstance(w, (bytes, bytearray, memoryview)):
        return bytes(w)
    if hasattr(w, "tobytes"):
        return w.tobytes()
    if bls:
        return b"".join(fr.bls_fr_mont(int(x) % fr.BLS_R) for x in w)
    return b"".join(fr.fr_mont(int(x) % fr.R) for x in w)


def _proof_bytes(p, nc: int, curve: str = "bn254") -> bytes:
    if isinstance(p, plonk_prover.Proof):
        if len(p.bsb22) != nc:
            raise ValueError(f"the proof has {len(p.bsb22)} BSB22 commitments, the key has {nc}")
        return plonk_prover.proof_bytes(p, curve)
    return bytes(p)


def verify_batch(proofs: Sequence, vk, witnesses: Sequence, challenge_hash: Optional[Callable] = None,
                 folding_hash: Optional[Callable] = None, host: bool = False) -> list:
    """plonk.Verify of every (proof, public witness) pair under vk (a VerifyingKey
    or a Bls12381VerifyingKey: the key's class chooses the curve): a list of
    VERIFY_* statuses.  A proof is a plonk_prover.Proof or its bytes in the
    library's layout; a witness is the public inputs as fr Montgomery bytes or as
    integers; challenge_hash / folding_hash: hashlib constructors (default
    SHA-256), as given to the prover.  host=True runs the same code on the CPU."""
    n = len(proofs)
    if n != len(witnesses):
        raise ValueError(f"{n} proofs, {len(witnesses)} witnesses")
    nc, nw = vk.n_commitments, vk.nb_public
    bls = _is_bls(vk)
    size = lib.gg_plonk_proof_size_ex(GG_CURVE_BLS12_381 if bls else GG_CURVE_BN254, nc)
    wb = [_witness_bytes(w, bls) for w in witnesses]
    pb = [_proof_bytes(p, nc, "bls12-381" if bls else "bn254") for p in proofs]
    for w in wb:
        if len(w) != 32 * nw:
            raise ValueError("invalid witness size")
    for i, p in enumerate(pb):
        if len(p) != size:
            raise ValueError(f"proof {i}: {len(p)} bytes, the key's proofs have {size}")
    packed, wit = b"".join(pb), b"".join(wb)
    status = bytearray(n)
    hc, hf = plonk_prover._hash_cb(challenge_hash), plonk_prover._hash_cb(folding_hash)
    if bls:
        fn = lib.gg_plonk_verify_batch_bls12_381_host if host else lib.gg_plonk_verify_batch_bls12_381
    else:
        fn = lib.gg_plonk_verify_batch_host if host else lib.gg_plonk_verify_batch
    check(fn(vk.handle, n, ptr(packed), ptr(wit) if nw else None, hc, None, hf, None, ptr(status)))
    return list(status)


def verify(proof, vk, public_witness, challenge_hash: Optional[Callable] = None,
           folding_hash: Optional[Callable] = None, host: bool = False) -> None:
    """plonk.Verify: returns None for a valid proof, raises VerifyError with
    gnark's message otherwise."""
    st = verify_batch([proof], vk, [public_witness], challenge_hash, folding_hash, host)[0]
    if st != VERIFY_OK:
        raise VerifyError(st)

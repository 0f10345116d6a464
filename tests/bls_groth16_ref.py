"""Synthetic Groth16 instances over BLS12-381 for the verifier tests (test
infrastructure; uses oracle/bls12_381_oracle.py): a verifying key built from
discrete logs (K_i = k_i G1, no circuit), with BSB22 commitments, and valid
proofs for any public witness.

With nc commitments the key carries a Pedersen key G = g G2,
GRootSigmaNeg = -(g / sigma) G2 and K has nc more points.  A proof carries
C_j = c_j G1; the hash of commitment j,

    h_j = fr.Hash(Marshal(C_j) | committed values (32 B big-endian), "bsb22-commitment"),

enters the public-input sum as the witness entry nb_public - 1 + j, and
pok = sigma sum_j r^j C_j with r = sha256("r" | h_0 | ...) mod r for two or more
commitments (r = 1 for one).  Krs is solved from the pairing equation

    a b = alpha beta + gamma (k_0 + sum_i x_i k_{i+1} + sum_j c_j) + delta krs."""
import hashlib
import random

import bls12_381_oracle as o

R = o.R
DST = b"bsb22-commitment"
OK, SUBGROUP, PEDERSEN, PAIRING = 0, 1, 2, 3


class Proof:
    """oracle points (None = the infinity)"""

    def __init__(self, ar, bs, krs, commitments=(), pok=None):
        self.ar, self.bs, self.krs, self.commitments, self.pok = ar, bs, krs, list(commitments), pok

    def replace(self, **kw):
        d = dict(ar=self.ar, bs=self.bs, krs=self.krs, commitments=self.commitments, pok=self.pok)
        d.update(kw)
        return Proof(**d)

    def gproof(self):
        from gnark_amd import groth16
        return groth16.Proof(o.g1_to_bytes(self.ar), o.g2_to_bytes(self.bs), o.g1_to_bytes(self.krs),
                             [o.g1_to_bytes(c) for c in self.commitments], o.g1_to_bytes(self.pok))


def commitment_hash(c, values) -> int:
    return o.hash_to_field(o.g1_raw_bytes(c) + b"".join(v.to_bytes(32, "big") for v in values), DST)


def fold_challenge(hashes) -> int:
    if len(hashes) < 2:
        return 1
    return int.from_bytes(hashlib.sha256(b"r" + b"".join(h.to_bytes(32, "big") for h in hashes)).digest(), "big") % R


class SyntheticKey:
    """nb_inputs public inputs (without the ONE wire) and nc commitments.
    Commitment 0 commits to the public input 1 (when there is one); commitment
    j > 0 to the public input 1 and to the hash wire of commitment j - 1.
    g1_multiples(ks) -> bytes may make the points k G1 elsewhere (the GPU).
    k_i = 0 for i in zero_k: K_i is the infinity, as for a public input that no
    constraint uses."""

    def __init__(self, nb_inputs: int, seed: int, nc: int = 0, g1_multiples=None, zero_k=()):
        rng = random.Random(seed)
        self.rng = rng
        self.alpha, self.beta, self.gamma, self.delta, self.g, self.sigma = (rng.randrange(1, R) for _ in range(6))
        self.nb_public, self.nc = nb_inputs + 1, nc
        self.k = [rng.randrange(1, R) for _ in range(self.nb_public + nc)]
        for i in zero_k:
            self.k[i] = 0
        if g1_multiples is None:
            self.K = [o.g1_mul(o.G1_GEN, k) for k in self.k]
        else:
            raw = bytes(g1_multiples(self.k))
            self.K = [o.g1_from_bytes(raw[96 * i:96 * i + 96]) for i in range(len(self.k))]
        first = [1] if nb_inputs else []
        self.committed = [first + ([self.nb_public + j - 1] if j else []) for j in range(nc)]

    def hashes(self, witness, commitments):
        """the hash wires of a proof's commitments under `witness`"""
        ext = list(witness)
        for j, c in enumerate(commitments):
            ext.append(commitment_hash(c, [ext[i - 1] for i in self.committed[j]]))
        return ext[len(witness):]

    def prove(self, witness, cs=None) -> Proof:
        """A valid proof for `witness`; cs: the commitments' discrete logs (0 = the infinity)."""
        assert len(witness) == self.nb_public - 1
        rng = self.rng
        cs = [rng.randrange(1, R) for _ in range(self.nc)] if cs is None else list(cs)
        assert len(cs) == self.nc
        cm = [o.g1_mul(o.G1_GEN, c) if c else o.INF for c in cs]
        hs = self.hashes(witness, cm)
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        s = (self.k[0] + sum(x * k for x, k in zip(list(witness) + hs, self.k[1:])) + sum(cs)) % R
        c = (a * b - self.alpha * self.beta - self.gamma * s) * pow(self.delta, -1, R) % R
        r = fold_challenge(hs)
        f = sum(pow(r, j, R) * cj for j, cj in enumerate(cs)) % R
        pok = o.g1_mul(o.G1_GEN, self.sigma * f % R) if self.nc and f else o.INF
        return Proof(o.g1_mul(o.G1_GEN, a), o.g2_mul(o.G2_GEN, b), o.g1_mul(o.G1_GEN, c) if c else o.INF, cm, pok)

    def prove_many(self, witnesses, g1_multiples, g2_multiples):
        """valid proofs for many witnesses of a key without commitments, the
        points a G1, c G1 and b G2 made in two batches by the given functions"""
        assert self.nc == 0
        rng, n = self.rng, len(witnesses)
        a = [rng.randrange(1, R) for _ in range(n)]
        b = [rng.randrange(1, R) for _ in range(n)]
        di = pow(self.delta, -1, R)
        c = []
        for w, ai, bi in zip(witnesses, a, b):
            assert len(w) == self.nb_public - 1
            s = (self.k[0] + sum(x * k for x, k in zip(w, self.k[1:]))) % R
            c.append((ai * bi - self.alpha * self.beta - self.gamma * s) * di % R)
        r1, r2 = bytes(g1_multiples(a + c)), bytes(g2_multiples(b))
        g1 = [o.g1_from_bytes(r1[96 * i:96 * i + 96]) for i in range(2 * n)]
        g2 = [o.g2_from_bytes(r2[192 * i:192 * i + 192]) for i in range(n)]
        return [Proof(g1[i], g2[i], g1[n + i]) for i in range(n)], (a, b, c)

    def vk_data(self):
        from gnark_amd import groth16
        kw = {}
        if self.nc:
            gs = self.g * pow(self.sigma, -1, R) % R
            kw = dict(commitment_key_g=o.g2_to_bytes(o.g2_mul(o.G2_GEN, self.g)),
                      commitment_key_g_root_sigma_neg=o.g2_to_bytes(o.g2_mul(o.G2_GEN, R - gs)),
                      public_and_commitment_committed=self.committed)
        return groth16.VerifyingKeyData(
            alpha1=o.g1_to_bytes(o.g1_mul(o.G1_GEN, self.alpha)), beta1=bytes(96), delta1=bytes(96),
            beta2=o.g2_to_bytes(o.g2_mul(o.G2_GEN, self.beta)), gamma2=o.g2_to_bytes(o.g2_mul(o.G2_GEN, self.gamma)),
            delta2=o.g2_to_bytes(o.g2_mul(o.G2_GEN, self.delta)), K=b"".join(o.g1_to_bytes(p) for p in self.K),
            nb_public=self.nb_public, curve="bls12-381", **kw)


def oracle_verify(key, proof, witness) -> bool:
    """the pairing equation of a key without commitments, by the big-integer reference pairing"""
    import bls_pairing_ref as br
    assert key.nc == 0
    g1, g2 = (lambda k: o.g1_mul(o.G1_GEN, k)), (lambda k: o.g2_mul(o.G2_GEN, k))
    case = dict(alpha=g1(key.alpha), beta=g2(key.beta), gamma=g2(key.gamma), delta=g2(key.delta), K=key.K,
                inputs=list(witness), ar=proof.ar, bs=proof.bs, krs=proof.krs)
    return br.pairing_product(br.groth16_pairs(case)).is_one()


_UNUSED = None


def unused_input_case():
    """A key with 2 public inputs whose K[2] is the infinity (input 2 is used by
    no constraint) and a batch of 4: two valid proofs whose dead input has every
    byte nonzero / is r - 1, the first proof with the dead input changed (still
    valid) and with the live input changed.  -> (key, proofs, witnesses, statuses),
    every status held against oracle_verify; made once per process."""
    global _UNUSED
    if _UNUSED is None:
        key = SyntheticKey(2, seed=77, zero_k=(2,))
        assert key.K[2] is o.INF and key.K[1] is not o.INF
        dead = int.from_bytes(bytes(range(0x11, 0x31)), "big")          # 32 nonzero bytes, < r
        wits = [[5, dead], [R - 2, R - 1], [5, dead ^ 0xFF00FF], [6, dead]]
        p1, p2 = key.prove(wits[0]), key.prove(wits[1])
        proofs, want = [p1, p2, p1, p1], [OK, OK, OK, PAIRING]
        for p, w, st in zip(proofs, wits, want):
            assert oracle_verify(key, p, w) == (st == OK)
        _UNUSED = key, proofs, wits, want
    return _UNUSED


def kat_vk_data(case):
    """VerifyingKeyData of one bellman vector (bls_pairing_ref.load_bellman_kats)"""
    from gnark_amd import groth16
    return groth16.VerifyingKeyData(
        alpha1=o.g1_to_bytes(case["alpha"]), beta1=bytes(96), delta1=bytes(96), beta2=o.g2_to_bytes(case["beta"]),
        gamma2=o.g2_to_bytes(case["gamma"]), delta2=o.g2_to_bytes(case["delta"]),
        K=b"".join(o.g1_to_bytes(p) for p in case["K"]), nb_public=len(case["K"]), curve="bls12-381")


def kat_proof(case) -> Proof:
    return Proof(case["ar"], case["bs"], case["krs"])


def kat_statuses(cases, host):
    """every bellman vector under its own key"""
    from gnark_amd import groth16
    out = []
    for c in cases:
        vk = groth16.Bls12381VerifyingKey(kat_vk_data(c))
        out += groth16.verify_batch([kat_proof(c).gproof()], vk, [c["inputs"]], host=host)
        vk.close()
    return out

"""Test helpers for the pairing and Groth16 Verify tests (test infrastructure;
uses the oracle): the E12 memory layout, an Fp2 square root, off-curve and
out-of-subgroup points, and synthetic Groth16 instances built from discrete
logs (a valid proof for any number of public inputs without a circuit)."""
import bn254_oracle as o

P, R = o.P, o.R
# position of the w^i coefficient in gnark-crypto's E12 layout
# (C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2) = (c0, c2, c4, c1, c3, c5)
E12_ORDER = (0, 2, 4, 1, 3, 5)
_E = None


def gt_to_bytes(f) -> bytes:
    """oracle Fp12 (coefficients of w^i) -> 384 bytes, Montgomery E2s in E12 order."""
    return b"".join(o.fp_to_bytes(f.c[i].a0) + o.fp_to_bytes(f.c[i].a1) for i in E12_ORDER)


def gt_from_bytes(b: bytes):
    c = [None] * 6
    for k, i in enumerate(E12_ORDER):
        c[i] = o.Fp2(o.fp_from_bytes(b[64 * k:64 * k + 32]), o.fp_from_bytes(b[64 * k + 32:64 * k + 64]))
    return o.Fp12(c)


def gt_one() -> bytes:
    return gt_to_bytes(o.Fp12.one())


def e_gen():
    """e(G1, G2), the reduced pairing of the generators (computed once)."""
    global _E
    if _E is None:
        _E = o.pairing(o.G1_GEN, o.G2_GEN)
    return _E


def e_power(k: int, multiple: int) -> bytes:
    """bytes of e(G1, G2)^(k * multiple)"""
    return gt_to_bytes(e_gen() ** (k * multiple % R))


def fp2_sqrt(a):
    """A square root of a in Fp2 = Fp[u]/(u^2 + 1), p = 3 mod 4, or None."""
    if a.is_zero():
        return a
    # norm-based: a = x + y u; alpha = sqrt(x^2 + y^2) in Fp
    x, y = a.a0, a.a1
    n = (x * x + y * y) % P
    alpha = pow(n, (P + 1) // 4, P)
    if alpha * alpha % P != n:
        return None
    for al in (alpha, P - alpha):
        d = (x + al) * pow(2, -1, P) % P
        s = pow(d, (P + 1) // 4, P)
        if s * s % P != d:
            continue
        if s == 0:
            continue
        t = y * pow(2 * s, -1, P) % P
        r = o.Fp2(s, t)
        if r * r == a:
            return r
    return None


def g2_on_twist(q) -> bool:
    x, y = q
    return y * y == x * x * x + o.B2


def g2_times_r(q):
    """r Q.  The oracle's g2_mul reduces its scalar mod r, so r Q is (r - 1) Q + Q."""
    return o.g2_add(o.g2_mul(q, R - 1), q)


def twist_point_outside_subgroup(seed: int):
    """A point of E'(Fp2) that is not in the r-torsion (the twist's cofactor is
    ~2^254, so a point found by a square root is outside with overwhelming
    probability; checked by multiplying with r)."""
    k = seed
    while True:
        x = o.Fp2(k, seed + 1)
        y = fp2_sqrt(x * x * x + o.B2)
        k += 1
        if y is None:
            continue
        q = (x, y)
        assert g2_on_twist(q)
        if g2_times_r(q) is not None:
            return q


def g2_off_twist(seed: int):
    q = o.g2_mul(o.G2_GEN, seed)
    bad = (q[0], q[1] + o.Fp2(1, 0))
    assert not g2_on_twist(bad)
    return bad


def g1_off_curve(seed: int):
    p = o.g1_mul(o.G1_GEN, seed)
    bad = (p[0], (p[1] + 1) % P)
    assert (bad[1] * bad[1] - bad[0] ** 3 - 3) % P != 0
    return bad


def proof_bytes(proof) -> bytes:
    return o.g1_to_bytes(proof.Ar) + o.g2_to_bytes(proof.Bs) + o.g1_to_bytes(proof.Krs)


class SyntheticKey:
    """A Groth16 verifying key from discrete logs: K_i = k_i G1, no circuit.
    k_i = 0 for i in zero_k: K_i is the infinity, as for a public input that no
    constraint uses."""

    def __init__(self, nb_inputs: int, seed: int, zero_k=()):
        rng = o.SplitMix64(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rng.fr() or 1 for _ in range(4))
        self.k = [rng.fr() for _ in range(nb_inputs + 1)]
        for i in zero_k:
            self.k[i] = 0
        self.rng = rng
        vk = o.VerifyingKey()
        vk.g1_alpha = o.g1_mul(o.G1_GEN, self.alpha)
        vk.g2_beta = o.g2_mul(o.G2_GEN, self.beta)
        vk.g2_gamma = o.g2_mul(o.G2_GEN, self.gamma)
        vk.g2_delta = o.g2_mul(o.G2_GEN, self.delta)
        import coracle
        pts = coracle.g1_batch_mul(o.g1_to_bytes(o.G1_GEN), o.fr_vec_to_bytes(self.k), len(self.k))
        vk.g1_K = [o.g1_from_bytes(bytes(pts[64 * i:64 * i + 64])) for i in range(len(self.k))]
        self.vk = vk
        self.nb_public = nb_inputs + 1

    def prove(self, witness):
        """A valid proof for `witness` (nb_public - 1 values): random a, b and
        Krs = ((a b - alpha beta - gamma sum x_i k_i) / delta) G1."""
        assert len(witness) == self.nb_public - 1
        a, b = self.rng.fr() or 1, self.rng.fr() or 1
        s = (self.k[0] + sum(x * k for x, k in zip(witness, self.k[1:]))) % R
        c = (a * b - self.alpha * self.beta - self.gamma * s) * pow(self.delta, -1, R) % R
        return o.Proof(o.g1_mul(o.G1_GEN, a), o.g2_mul(o.G2_GEN, b), o.g1_mul(o.G1_GEN, c))

    def vk_data(self):
        from gnark_amd import groth16
        vk = self.vk
        return groth16.VerifyingKeyData(
            alpha1=o.g1_to_bytes(vk.g1_alpha), beta1=bytes(64), delta1=bytes(64), beta2=o.g2_to_bytes(vk.g2_beta),
            gamma2=o.g2_to_bytes(vk.g2_gamma), delta2=o.g2_to_bytes(vk.g2_delta),
            K=b"".join(o.g1_to_bytes(p) for p in vk.g1_K), nb_public=self.nb_public)


def vk_data_from_oracle(vk, nb_public, bsb22=False):
    """VerifyingKeyData of an oracle key (bn254_oracle.setup / bn254_bsb22.setup_bsb22)."""
    from gnark_amd import groth16
    kw = {}
    if bsb22:
        kw = dict(commitment_key_g=o.g2_to_bytes(vk.commitment_key.g),
                  commitment_key_g_root_sigma_neg=o.g2_to_bytes(vk.commitment_key.g_root_sigma_neg),
                  public_and_commitment_committed=[list(c) for c in vk.public_committed])
    return groth16.VerifyingKeyData(
        alpha1=o.g1_to_bytes(vk.g1_alpha), beta1=bytes(64), delta1=bytes(64), beta2=o.g2_to_bytes(vk.g2_beta),
        gamma2=o.g2_to_bytes(vk.g2_gamma), delta2=o.g2_to_bytes(vk.g2_delta),
        K=b"".join(o.g1_to_bytes(p) for p in vk.g1_K), nb_public=nb_public, **kw)

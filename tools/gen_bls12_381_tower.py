"""Prints the constant tables of Bls12381Tower (csrc/pairing.cuh): the Frobenius
coefficients xi^(i (p^k - 1) / 6), xi = 1 + u, for k = 1, 2, 3 and i = 1..5, and
the twist coefficient 4 xi, as {a0, a1} pairs of twelve 32-bit Montgomery limbs
(R = 2^384), least significant limb first; then the constants of the
endomorphism membership checks: the cube root of unity BETA of
phi(x, y) = (BETA x, y) with [x^2] phi(P) + P = 0 on G1 (of the two primitive
roots the one for which the generator passes), and the two Fp2 constants of
psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y), the untwist-Frobenius-twist map of
the M-type twist, 1 / xi^((p - 1) / 3) and 1 / xi^((p - 1) / 2), checked by
psi(G2) = [x] G2.

    python tools/gen_bls12_381_tower.py            # the tower's tables
    python tools/gen_bls12_381_tower.py --endo     # BETA and PSI
"""
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X = -0xD201000000010000
LIMBS = 12


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


class Field:
    """the operations the affine group law needs, over Fp (ints) or Fp2 (pairs)"""

    def __init__(self, mul, inv, sub, scale):
        self.mul, self.inv, self.sub, self.scale = mul, inv, sub, scale


FP = Field(lambda a, b: a * b % P, lambda a: pow(a, -1, P), lambda a, b: (a - b) % P, lambda a, k: a * k % P)
FP2 = Field(f2_mul, f2_inv, lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P),
            lambda a, k: (a[0] * k % P, a[1] * k % P))


def ec_add(f, p, q):
    """affine addition on y^2 = x^3 + b (None is the infinity)"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == f.sub(p[1], p[1]):
            return None
        lam = f.mul(f.scale(f.mul(p[0], p[0]), 3), f.inv(f.scale(p[1], 2)))
    else:
        lam = f.mul(f.sub(q[1], p[1]), f.inv(f.sub(q[0], p[0])))
    x = f.sub(f.sub(f.mul(lam, lam), p[0]), q[0])
    return (x, f.sub(f.mul(lam, f.sub(p[0], x)), p[1]))


def ec_mul(f, p, k):
    assert k >= 0
    r = None
    while k:
        if k & 1:
            r = ec_add(f, r, p)
        p = ec_add(f, p, p)
        k >>= 1
    return r


G1 = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
      0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


def endo_beta():
    """the primitive cube root of unity with [x^2] (beta x, y) + (x, y) = 0 at the generator"""
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    b = pow(g, (P - 1) // 3, P)
    good = [c for c in (b, b * b % P)
            if ec_add(FP, ec_mul(FP, (c * G1[0] % P, G1[1]), X * X), G1) is None]
    assert len(good) == 1
    return good[0]


def endo_psi():
    """(PSI_X, PSI_Y): psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y), psi(G2) = [x] G2, x < 0"""
    cx = f2_inv(f2_pow((1, 1), (P - 1) // 3))
    cy = f2_inv(f2_pow((1, 1), (P - 1) // 2))
    conj = lambda a: (a[0], -a[1] % P)
    psi = (f2_mul(conj(G2[0]), cx), f2_mul(conj(G2[1]), cy))
    xq = ec_mul(FP2, G2, -X)
    assert psi == (xq[0], FP2.sub((0, 0), xq[1]))
    return cx, cy


def limbs(x):
    m = x * (1 << (32 * LIMBS)) % P
    return [(m >> (32 * i)) & 0xFFFFFFFF for i in range(LIMBS)]


def row(a):
    w = limbs(a[0]) + limbs(a[1])
    lines = [", ".join("0x%08xu" % v for v in w[i:i + 8]) for i in range(0, len(w), 8)]
    return "    {" + ",\n     ".join(lines) + "}"


def main():
    assert R == X ** 4 - X ** 2 + 1 and 3 * P == (X - 1) ** 2 * R + 3 * X
    # the final exponentiation's multiple: 3 Phi_12(p) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3
    assert 3 * (P ** 4 - P ** 2 + 1) == R * ((X - 1) ** 2 * (X + P) * (X * X + P * P - 1) + 3)
    for k in (1, 2, 3):
        assert (P ** k - 1) % 6 == 0
        print("    // xi^(i (p^%d - 1) / 6), i = 1..5, {a0, a1} Montgomery limbs" % k)
        print("    static constexpr uint32_t G%dC[5][24] = {" % k)
        print(",\n".join(row(f2_pow((1, 1), i * (P ** k - 1) // 6)) for i in range(1, 6)) + "};")
    print("    // twist coefficient b' = 4 xi")
    print("    static constexpr uint32_t BT[24] =")
    print(row((4, 4)) + ";")


def main_endo():
    print("    // phi(x, y) = (BETA x, y): [x^2] phi(P) + P = 0 on G1")
    print("    static constexpr uint32_t BETA[12] =")
    w = limbs(endo_beta())
    print("    {" + ",\n     ".join(", ".join("0x%08xu" % v for v in w[i:i + 8]) for i in range(0, 12, 8)) + "};")
    cx, cy = endo_psi()
    print("    // psi(x, y) = (conj(x) PSI[0], conj(y) PSI[1]): psi(Q) = [x] Q on G2")
    print("    static constexpr uint32_t PSI[2][24] = {")
    print(row(cx) + ",\n" + row(cy) + "};")


if __name__ == "__main__":
    import sys
    if "--endo" in sys.argv[1:]:
        main_endo()
    else:
        main()

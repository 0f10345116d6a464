"""Test infrastructure of the point codec tests (test_point_codec_cpu.py,
test_gpu_point_codec.py): per group, points with their reference encodings from
the existing Python codecs (gnark_amd.pkio for BN254, oracle/bls12_381_oracle.py
for BLS12-381), the inputs of the square-root tests with Euler's criterion from
big integers, and one malformed input per status.  Everything is computed once
per process and never changed."""
import functools
import random

import bls12_381_oracle as bls
import bls_pairing_ref as bref
import bn254_oracle as bn

OK, NOT_ON_CURVE, NOT_IN_SUBGROUP, BAD_ENCODING = 0, 1, 2, 3
N_POINTS = 257


class Group:
    def __init__(self, name, gid, curve, g, fb):
        self.name, self.gid, self.curve, self.g, self.fb = name, gid, curve, g, fb
        self.pt = 2 * g * fb              # affine Montgomery bytes
        self.bls = curve == "bls12-381"
        self.p = bls.P if self.bls else bn.P

    def esz(self, raw):
        return self.g * self.fb * (2 if raw else 1)

    # ---- points as the oracles hold them <-> Montgomery bytes
    def to_bytes(self, p):
        if self.bls:
            return (bls.g1_to_bytes if self.g == 1 else bls.g2_to_bytes)(p)
        return (bn.g1_to_bytes if self.g == 1 else bn.g2_to_bytes)(p)

    def coords(self, p):
        """canonical integers (x, y) or ((x0, x1), (y0, y1))"""
        if self.g == 1 or self.bls:
            return p
        return ((p[0].a0, p[0].a1), (p[1].a0, p[1].a1))

    def from_coords(self, c):
        if self.g == 1 or self.bls:
            return c
        return (bn.Fp2(*c[0]), bn.Fp2(*c[1]))

    # ---- the reference encoders
    def encode(self, p, raw):
        if not self.bls:
            from gnark_amd import pkio
            return (pkio._g1_encode if self.g == 1 else pkio._g2_encode)(self.to_bytes(p), raw)
        if not raw:
            return (bls.g1_compress if self.g == 1 else bls.g2_compress)(p)
        if self.g == 1:
            return bls.g1_raw_bytes(p)
        if p is bls.INF:  # G2Affine.RawBytes: X.A1 | X.A0 | Y.A1 | Y.A0, mUncompressedInfinity as on G1
            return bytes([0x40]) + bytes(191)
        return b"".join(v.to_bytes(48, "big") for v in (p[0][1], p[0][0], p[1][1], p[1][0]))

    def raw_of_coords(self, c):
        """raw bytes of coordinates that need not be on the curve"""
        if self.g == 1:
            return c[0].to_bytes(self.fb, "big") + c[1].to_bytes(self.fb, "big")
        return b"".join(v.to_bytes(self.fb, "big") for v in (c[0][1], c[0][0], c[1][1], c[1][0]))

    def compressed_of_x(self, x, largest=False):
        """compressed bytes naming x (an int, or (x0, x1)) whether or not it has a y"""
        b = bytearray(x.to_bytes(self.fb, "big") if self.g == 1 else
                      x[1].to_bytes(self.fb, "big") + x[0].to_bytes(self.fb, "big"))
        b[0] |= (0xA0 if self.bls else 0xC0) if largest else 0x80
        return bytes(b)

    # ---- field arithmetic on canonical integers, for the searches
    def rhs(self, x):
        """x^3 + b as an int (G1) or (a0, a1) (G2)"""
        p = self.p
        if self.g == 1:
            return (x ** 3 + (4 if self.bls else 3)) % p
        b2 = bls.B2 if self.bls else (bn.B2.a0, bn.B2.a1)
        x3 = f2_mul(f2_mul(x, x, p), x, p)
        return ((x3[0] + b2[0]) % p, (x3[1] + b2[1]) % p)

    def is_square(self, a):
        p = self.p
        n = a % p if self.g == 1 else (a[0] * a[0] + a[1] * a[1]) % p
        return n == 0 or pow(n, (p - 1) // 2, p) == 1


def f2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def _groups():
    from gnark_amd import _lib
    return {g.name: g for g in (Group("bn254-g1", _lib.GG_G1, "bn254", 1, 32),
                                Group("bn254-g2", _lib.GG_G2, "bn254", 2, 32),
                                Group("bls12-381-g1", _lib.GG_BLS12_381_G1, "bls12-381", 1, 48),
                                Group("bls12-381-g2", _lib.GG_BLS12_381_G2, "bls12-381", 2, 48))}


GROUP_NAMES = ("bn254-g1", "bn254-g2", "bls12-381-g1", "bls12-381-g2")


@functools.lru_cache(maxsize=None)
def group(name):
    return _groups()[name]


@functools.lru_cache(maxsize=None)
def points(name):
    """N_POINTS points of the group: random multiples of the generator (k G + i s G),
    the infinity at indices 0 and 64."""
    g = group(name)
    rng = random.Random("codec-" + name)
    if g.bls:
        mul, add, gen, mod = (bls.g1_mul, bls.g1_add, bls.G1_GEN, bls.R) if g.g == 1 else \
            (bls.g2_mul, bls.g2_add, bls.G2_GEN, bls.R)
    else:
        mul, add, gen, mod = (bn.g1_mul, bn.g1_add, bn.G1_GEN, bn.R) if g.g == 1 else \
            (bn.g2_mul, bn.g2_add, bn.G2_GEN, bn.R)
    p, step = mul(gen, rng.randrange(1, mod)), mul(gen, rng.randrange(1, mod))
    out = []
    for i in range(N_POINTS):
        out.append(None if i in (0, 64) else p)
        p = add(p, step)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def encoded(name, raw, n=N_POINTS):
    """(Montgomery bytes, reference encoding) of the first n points"""
    g = group(name)
    pts = points(name)[:n]
    return b"".join(g.to_bytes(p) for p in pts), b"".join(g.encode(p, raw) for p in pts)


# ---------------------------------------------------------------- square roots
@functools.lru_cache(maxsize=None)
def sqrt_inputs(curve, degree):
    """(Montgomery bytes, canonical values, expected ok) of 0, 1, -1, the squares
    of 32 random elements and 32 random elements"""
    p, fb = (bn.P, 32) if curve == "bn254" else (bls.P, 48)
    rng = random.Random(f"sqrt-{curve}-{degree}")
    mont = lambda x: (x * (1 << (8 * fb)) % p).to_bytes(fb, "little")
    if degree == 1:
        vals = [0, 1, p - 1] + [rng.randrange(p) ** 2 % p for _ in range(32)] + [rng.randrange(p) for _ in range(32)]
        ok = [int(a == 0 or pow(a, (p - 1) // 2, p) == 1) for a in vals]
        return b"".join(mont(a) for a in vals), vals, ok
    rnd = lambda: (rng.randrange(p), rng.randrange(p))
    vals = [(0, 0), (1, 0), (p - 1, 0)]
    for _ in range(32):
        a = rnd()
        vals.append(f2_mul(a, a, p))
    vals += [rnd() for _ in range(32)]
    vals += [(rng.randrange(p) ** 2 % p, 0), ((p - rng.randrange(1, p) ** 2) % p, 0)]  # Fp: a residue, a non-residue
    ok = []
    for a in vals:  # Euler's criterion on the norm
        n = (a[0] * a[0] + a[1] * a[1]) % p
        ok.append(int(n == 0 or pow(n, (p - 1) // 2, p) == 1))
    return b"".join(mont(a[0]) + mont(a[1]) for a in vals), vals, ok


def unmont(b, curve):
    p, fb = (bn.P, 32) if curve == "bn254" else (bls.P, 48)
    return int.from_bytes(b, "little") * pow(1 << (8 * fb), -1, p) % p


# ---------------------------------------------------------------- malformed inputs
def _outside_subgroup(g):
    """a point on the curve outside the order-r subgroup, or None (BN254 G1 has no cofactor)"""
    if g.bls:
        return bref.g1_outside_subgroup() if g.g == 1 else bref.twist_point_outside_subgroup(5)
    if g.g == 1:
        return None
    from gnark_amd import pkio
    k = 5
    while True:  # the search of bls_pairing_ref.twist_point_outside_subgroup on BN254's twist
        x = (k, 6)
        k += 1
        y = pkio._f2_sqrt(g.rhs(x))
        if y is None:
            continue
        q = g.from_coords((x, y))
        assert bn.on_curve_g2(q)
        F = bn._Fp2Ops
        base, acc = bn.jac_from_affine(F, q), (F.one, F.one, F.zero)
        for bit in bin(bn.R)[2:]:  # r Q by plain double-and-add (jac_mul reduces its scalar mod r)
            acc = bn.jac_double(F, acc)
            if bit == "1":
                acc = bn.jac_add(F, acc, base)
        if not bn.jac_is_inf(F, acc):
            return q


@functools.lru_cache(maxsize=None)
def bad_cases(name):
    """[(label, raw, encoded bytes, status with checks, status without, Montgomery
    bytes when decoded without checks or None)] -- one input per status"""
    g = group(name)
    good = points(name)[1]
    c = g.coords(good)
    cases = []
    comp, rawb = g.encode(good, False), g.encode(good, True)
    if g.bls:
        for flag in (0x20, 0x60, 0xE0):  # 001, 011, 111
            b = bytearray(comp)
            b[0] = (b[0] & 0x1F) | flag
            cases.append((f"invalid flag {flag >> 5:03b}", False, bytes(b), BAD_ENCODING, BAD_ENCODING, None))
    xp = g.p if g.g == 1 else (c[0][0], g.p)  # the first coordinate on the wire = p
    cases.append(("coordinate = p, compressed", False, g.compressed_of_x(xp), BAD_ENCODING, BAD_ENCODING, None))
    yp = (c[0], g.p) if g.g == 1 else (c[0], (g.p, c[1][1]))
    cases.append(("coordinate = p, raw", True, g.raw_of_coords(yp), BAD_ENCODING, BAD_ENCODING, None))
    b = bytearray(rawb)
    b[0] |= 0x80
    cases.append(("compressed flag in a raw call", True, bytes(b), BAD_ENCODING, BAD_ENCODING, None))
    cases.append(("raw point in a compressed call", False, rawb[:g.esz(False)], BAD_ENCODING, BAD_ENCODING, None))
    k = 1
    while True:  # a small x with no y
        x = k if g.g == 1 else (k, 1)
        if not g.is_square(g.rhs(x)):
            break
        k += 1
    cases.append(("x with no y", False, g.compressed_of_x(x), NOT_ON_CURVE, NOT_ON_CURVE, None))
    y1 = (c[0], (c[1] + 1) % g.p) if g.g == 1 else (c[0], ((c[1][0] + 1) % g.p, c[1][1]))
    cases.append(("raw point with y + 1", True, g.raw_of_coords(y1), NOT_ON_CURVE, None, None))
    out = _outside_subgroup(g)
    if out is not None:
        for raw in (False, True):
            cases.append((f"outside the subgroup, {'raw' if raw else 'compressed'}", raw, g.encode(out, raw),
                          NOT_IN_SUBGROUP, OK, g.to_bytes(out)))
    return tuple(cases)

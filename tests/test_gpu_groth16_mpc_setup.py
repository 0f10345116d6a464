"""Groth16 keys from a powers-of-tau SRS on the GPU (gnark_amd.mpcsetup,
gg_groth16_setup_from_srs / gg_groth16_setup_contribute, gg_kzg_to_lagrange_g2;
backend/groth16/bn254/mpcsetup/phase2.go:53-210, setup.go:25-97), bit-exact.

The yardstick: with gamma = 1, the key extracted from an SRS built from a known
(tau, alpha, beta), after contributions whose product is delta, is byte for byte
the key groth16.setup makes from (tau, alpha, beta, 1, delta).  That function is
pinned to the oracles by tests/test_gpu_groth16_setup.py; the cubic tests here
compare with the oracles directly.  No tolerance anywhere: affine coordinates
are unique."""
import dataclasses
import functools
import random

import pytest

import bls12_381_oracle as bls
import bn254_oracle as o
import r1cs_solver

pytestmark = pytest.mark.gpu

CURVES = ("bn254", "bls12-381")
TAU, ALPHA, BETA = 0x1DEA5EED1234567, 0xA1FA0001, 0xBE7A0002
D1, D2 = 0xDE17A0003, 0x5EC0DDE17A


def _mod(curve):
    return o.R if curve == "bn254" else bls.R


@functools.lru_cache(maxsize=None)
def _srs(curve, power):
    """the single-party SRS of 2^power, built once per size and left unchanged"""
    from gnark_amd import mpcsetup
    return mpcsetup.srs_from_trapdoor(power, TAU, ALPHA, BETA, curve)


def _tw(delta, curve):
    from gnark_amd import groth16
    return groth16.ToxicWaste(TAU % _mod(curve), ALPHA, BETA, 1, delta % _mod(curve))


def _same_keys(got, want):
    """every field of (ProvingKeyData, VerifyingKeyData)"""
    for g, w in zip(got, want):
        assert type(g) is type(w)
        for f in dataclasses.fields(g):
            a, b = getattr(g, f.name), getattr(w, f.name)
            if isinstance(a, (bytes, bytearray)):
                a, b = bytes(a), bytes(b)
            assert a == b, f"{type(g).__name__}.{f.name} differs"


def _power(ncons):
    return max(ncons - 1, 0).bit_length()


def _from_csr(curve, nb_public, nw, off, wires, cids, table, deltas=(D1,), power=None, **kw):
    """(keys from the SRS after the contributions, the Phase2 info, Setup's keys for their product)"""
    from gnark_amd import groth16, mpcsetup
    ncons = (len(off) - 1) // 3
    srs = _srs(curve, _power(ncons) if power is None else power)
    p2 = mpcsetup.init_phase2(nb_public, nw, off, wires, cids, table, srs, **kw)
    prod = 1
    for d in deltas:
        p2.contribute(d)
        prod = prod * d % _mod(curve)
    got = p2.extract_keys()
    info = (p2.log_n, p2.acc_chunk, p2.acc_launches, p2.timings())
    p2.close()
    want = groth16.setup(nb_public, nw, off, wires, cids, table, toxic_waste=_tw(prod, curve), curve=curve)
    return got, info, want


# ---------------------------------------------------------------- 1, 2. cubic against the oracles
def _cat(f, pts):
    return b"".join(f(p) for p in pts)


def test_cubic_bn254_every_field_against_the_oracle():
    """InitPhase2 + ExtractKeys against oracle/bn254_oracle.py:setup with gamma = 1,
    delta = 1 (no GPU Setup in between), then two contributions."""
    from gnark_amd import mpcsetup
    rcs = o.cubic_r1cs()
    p2 = mpcsetup.init_phase2_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, _srs("bn254", 2))
    delta = 1
    for step in (None, D1, D2):
        if step is not None:
            p2.contribute(step)
            delta = delta * step % o.R
        pk, vk = p2.extract_keys()
        rp, rv = o.setup(rcs, o.ToxicWaste(TAU, ALPHA, BETA, 1, delta))
        g1, g2 = o.g1_to_bytes, o.g2_to_bytes
        assert pk.log_n == 2 and pk.nb_public == 2 and pk.k_wire_index is None and pk.commitment_keys is None
        assert pk.g1_A == _cat(g1, rp.g1_A) and pk.g1_B == _cat(g1, rp.g1_B) and pk.g2_B == _cat(g2, rp.g2_B)
        assert pk.g1_K == _cat(g1, rp.g1_K) and pk.g1_Z == _cat(g1, rp.g1_Z) and len(rp.g1_Z) == 3
        assert (pk.alpha1, pk.beta1, pk.delta1) == (g1(rp.g1_alpha), g1(rp.g1_beta), g1(rp.g1_delta))
        assert (pk.beta2, pk.delta2) == (g2(rp.g2_beta), g2(rp.g2_delta))
        assert bytes(pk.infinity_A) == bytes(map(int, rp.infinity_A))
        assert bytes(pk.infinity_B) == bytes(map(int, rp.infinity_B))
        assert vk.K == _cat(g1, rv.g1_K) and vk.gamma2 == g2(rv.g2_gamma) == g2(o.G2_GEN)
        assert (vk.alpha1, vk.beta1, vk.delta1, vk.beta2, vk.delta2) == \
            (pk.alpha1, pk.beta1, pk.delta1, pk.beta2, pk.delta2)
        assert vk.commitment_key_g is None and list(vk.public_and_commitment_committed) == []
    p2.close()


def test_cubic_bls12_381_against_the_oracle_scalars():
    from gnark_amd import mpcsetup
    rcs = o.cubic_r1cs()
    p2 = mpcsetup.init_phase2_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, _srs("bls12-381", 2))
    p2.contribute(D1)
    pk, vk = p2.extract_keys()
    p2.close()
    t = TAU % bls.R
    ks = bls.groth16_setup_scalars(rcs.constraints, rcs.nb_wires, rcs.nb_public, 2, t, ALPHA, BETA, D1)
    g1 = lambda xs: b"".join(bls.g1_to_bytes(bls.g1_mul(bls.G1_GEN, x)) for x in xs)
    g2 = lambda xs: b"".join(bls.g2_to_bytes(bls.g2_mul(bls.G2_GEN, x)) for x in xs)
    assert pk.curve == "bls12-381" and pk.log_n == 2
    assert pk.g1_A == g1(ks["A"]) and pk.g1_B == g1(ks["B"]) and pk.g2_B == g2(ks["B"])
    assert pk.g1_K == g1(ks["K"]) and pk.g1_Z == g1(ks["Z"])
    assert bytes(pk.infinity_A) == bytes(ks["infA"]) and bytes(pk.infinity_B) == bytes(ks["infB"])
    vkk = [(ks["u"][i] * BETA + ks["v"][i] * ALPHA + ks["w"][i]) % bls.R for i in range(rcs.nb_public)]  # gamma = 1
    assert vk.K == g1(vkk)
    assert pk.alpha1 + pk.beta1 + pk.delta1 == g1([ALPHA, BETA, D1])
    assert pk.beta2 + pk.delta2 + vk.gamma2 == g2([BETA, D1, 1])


# ---------------------------------------------------------------- 3. random systems
@pytest.mark.parametrize("curve,seed", [("bn254", 1), ("bls12-381", 3)])
def test_random_systems(curve, seed):
    """domain 1024, ~710 wires (several blocks); random coefficients: nearly every term is general"""
    from gnark_amd import groth16
    rng = random.Random(8800 + seed)
    nb_public, nb_secret, n_int = 3, 5, 700 + seed
    cons = r1cs_solver.random_circuit(rng, nb_public, nb_secret, n_int, R=_mod(curve))
    off, wires, cids, table = groth16.terms_to_csr(cons, _mod(curve))
    got, info, want = _from_csr(curve, nb_public, nb_public + nb_secret + n_int, off, wires, cids, table)
    assert info[0] == 10
    _same_keys(got, want)


# ---------------------------------------------------------------- 4. hand-built edges
def _edge_sides(C, ncons, ids):
    """test_gpu_groth16_setup.test_edge_system's construction over coefficient ids
    ids = (zero, one, two, minus_one, general...)"""
    ZERO, ONE, TWO, M1, K, K3, KM2, KBIG = ids
    PM, DUP, DM1, DC, DP1, DSQ, ZERO_ID, GEN, FREE = 2, 3, 4, 5, 6, 7, 8, 9, 10
    nw = FREE + 20
    assert C * C + 1 <= 3 * ncons
    sides = [[[(0, ONE)], [], []] for _ in range(ncons)]  # wire 0, coefficient 1, in L of EVERY constraint
    for j in range(ncons):
        sides[j][2].append((FREE + j % 20, ONE))          # wires absent from every R
    sides[5][0] += [(PM, ONE), (PM, M1)]                  # +1 and -1 on one constraint: A[PM] = infinity by value
    sides[7][1] += [(DUP, ONE), (DUP, ONE)]               # the same (constraint, +1) term twice: a doubling
    sides[8][1] += [(DUP, TWO), (DUP, M1)]                # 2 and -1 in one side
    sides[9][1] += [(ZERO_ID, ZERO)]                      # a zero coefficient on an otherwise absent wire
    sides[11][0] += [(GEN, K3), (GEN, KM2), (GEN, KBIG)]  # 3, r - 2 and one above 2^253
    sides[12][1] += [(GEN, K3), (GEN, KBIG)]
    for j in range(C - 1):
        sides[j][2].append((DM1, K))                      # degree chunk - 1
    for j in range(C):
        sides[100 + j][2].append((DC, K))                 # degree chunk
    for j in range(C + 1):
        sides[200 + j][1].append((DP1, K))                # degree chunk + 1
    left = C * C + 1                                      # degree chunk^2 + 1: up to three per constraint
    for j in range(ncons):
        for _ in range(min(3, left)):
            sides[j][1].append((DSQ, K))
            left -= 1
    assert left == 0
    off, wires, cids = [0], [], []
    for s3 in sides:
        for side in s3:
            wires += [w for w, _ in side]
            cids += [c for _, c in side]
            off.append(len(wires))
    return nw, off, wires, cids, (PM, DUP, ZERO_ID, FREE)


@pytest.mark.parametrize("numbering", ["gnark", "shuffled"])
def test_edge_system(numbering):
    """512 constraints = the whole domain; degrees chunk - 1, chunk, chunk + 1,
    chunk^2 + 1; cancellation, doubling, a zero coefficient.  Twice: with gnark's
    ids 0..3 = 0, 1, 2, -1, and with general values at ids 0..3 and 0, 1, 2, -1 at
    higher ids -- the second fails if anything keys on the id."""
    from gnark_amd import mpcsetup
    ncons, nb_public = 512, 2
    K, KBIG = 0x1234567890ABCDEF, (1 << 253) + 0x123456789
    assert KBIG < o.R
    tiny = mpcsetup.init_phase2(2, 5, [0, 1, 2, 3], [2, 2, 3], [0, 0, 0], [1], _srs("bn254", 0))
    C = tiny.acc_chunk
    tiny.close()
    assert C >= 2
    if numbering == "gnark":
        table = [0, 1, 2, o.R - 1, K, 3, o.R - 2, KBIG]
        ids = (0, 1, 2, 3, 4, 5, 6, 7)
    else:
        table = [K, 3, o.R - 2, KBIG, 2, 0, o.R - 1, 1]
        ids = (5, 7, 4, 6, 0, 1, 2, 3)
    nw, off, wires, cids, (PM, DUP, ZERO_ID, FREE) = _edge_sides(C, ncons, ids)
    (pk, vk), info, want = _from_csr("bn254", nb_public, nw, off, wires, cids, table)
    assert info[0] == 9 and info[1] == C
    assert info[3]["general_terms"] == (C - 1) + C + (C + 1) + (C * C + 1) + 5
    # A[0] = sum_j L_j(tau) = 1: the first G1.A point is the generator (needs no oracle)
    assert pk.g1_A[:64] == o.g1_to_bytes(o.G1_GEN)
    assert pk.infinity_A[0] == 0 and pk.infinity_A[PM] == 1 and pk.infinity_B[DUP] == 0
    assert pk.infinity_B[ZERO_ID] == 1 and all(pk.infinity_B[FREE:])
    _same_keys((pk, vk), want)


# ---------------------------------------------------------------- 5. MiMC shape
def test_mimc_shape_three_rounds():
    """2^12: wire 0 carries 1,360 O-side terms, every one with a general coefficient"""
    from test_gpu_solver import mimc_csr
    m = mimc_csr(1 << 4, 85, 1)
    got, info, want = _from_csr("bn254", m["nb_public"], m["nw"], m["off"], m["wires"], m["coef"], m["table"])
    log_n, chunk, launches, tm = info
    assert log_n == 12
    assert chunk <= 36 and 1360 > chunk ** 2  # three rounds for wire 0 in the first accumulation
    assert launches >= 3 + 1 + 1              # and at least one launch for each of the other two
    assert tm["general_terms"] == 1360 and tm["terms"] == len(m["wires"])
    _same_keys(got, want)


# ---------------------------------------------------------------- 6. SRS size, device buffers, one constraint
def _cubic_csr(curve):
    from gnark_amd import groth16
    rcs = o.cubic_r1cs()
    return (rcs.nb_public, rcs.nb_wires) + tuple(groth16.terms_to_csr(rcs.constraints, _mod(curve)))


@pytest.mark.parametrize("curve", CURVES)
def test_larger_srs_and_device_buffers(curve):
    from gnark_amd import mpcsetup
    from gnark_amd._lib import DeviceBuffer
    args = _cubic_csr(curve)
    got, _, want = _from_csr(curve, *args)
    _same_keys(got, want)
    big, _, _ = _from_csr(curve, *args, power=4)  # N = 4 n: the prefixes are used
    _same_keys(big, want)
    s = _srs(curve, 4)
    dev = mpcsetup.Phase1Srs(*(DeviceBuffer.from_host(p) for p in (s.tau_g1, s.alpha_tau_g1, s.beta_tau_g1, s.tau_g2,
                                                                   s.beta_g2)), n=s.n, curve=curve)
    p2 = mpcsetup.init_phase2(*args, dev)
    p2.contribute(D1)
    _same_keys(p2.extract_keys(), want)
    p2.close()
    assert dev.tau_g1.to_host() == s.tau_g1 and dev.tau_g2.to_host() == s.tau_g2  # the inputs are left alone


@pytest.mark.parametrize("curve", CURVES)
def test_one_constraint(curve):
    """log_n = 0: no Z, the Lagrange form of one point is the point"""
    got, info, want = _from_csr(curve, 2, 5, [0, 1, 2, 3], [2, 3, 4], [0, 1, 0], [1, 7])
    assert info[0] == 0 and got[0].g1_Z == b""
    _same_keys(got, want)


# ---------------------------------------------------------------- 7. the loop closes
@pytest.mark.parametrize("curve", CURVES)
def test_setup_from_srs_prove_verify(curve):
    from gnark_amd import backend, groth16, mpcsetup, solver
    rcs = o.cubic_r1cs()
    p2 = mpcsetup.init_phase2_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, _srs(curve, 2))
    p2.contribute()  # a sampled delta: nobody keeps it
    pkd, vkd = p2.extract_keys()
    p2.close()
    pk = groth16.ProvingKey(pkd)
    sys_ = solver.R1CS.from_terms(rcs.nb_public, rcs.nb_secret, rcs.nb_wires, rcs.constraints, curve=curve)
    proof = groth16.prove(pk, sys_.solve([35, 3]), backend.with_amd_acceleration())
    sys_.close()
    pk.close()
    vk = groth16.VerifyingKey(vkd) if curve == "bn254" else groth16.Bls12381VerifyingKey(vkd)
    groth16.verify(proof, vk, [35])
    with pytest.raises(groth16.VerifyError, match="pairing doesn't match"):
        groth16.verify(proof, vk, [36])
    vk.close()


# ---------------------------------------------------------------- 8. the EC-NTT over G2
def _g2(curve):
    """(add, mul, to_bytes, generator, bytes per point, batch_scalar_mul group) of the oracle's G2"""
    from gnark_amd import msm
    if curve == "bn254":
        return o.g2_add, o.g2_mul, o.g2_to_bytes, o.G2_GEN, 128, msm.G2
    return bls.g2_add, bls.g2_mul, bls.g2_to_bytes, bls.G2_GEN, 192, msm.BLS12_381_G2


def _omega(curve, log_n):
    from gnark_amd import fr
    return (fr.domain_generator if curve == "bn254" else fr.bls_domain_generator)(log_n)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [1, 2, 3])
def test_to_lagrange_g2_small_against_the_oracle_dft(curve, log_n):
    """out[i] = (1/n) sum_j omega^(-ij) in[j] over the oracle's G2 arithmetic, an infinity among the inputs"""
    from gnark_amd import kzg
    add, mul, tob, gen, _, _ = _g2(curve)
    mod, n = _mod(curve), 1 << log_n
    rng = random.Random(4100 + log_n)
    pts = [mul(gen, rng.randrange(1, mod)) for _ in range(n)]
    pts[n - 1] = mul(gen, 0)  # the point at infinity
    assert tob(pts[n - 1]) == bytes(len(tob(gen)))
    winv, ninv = pow(_omega(curve, log_n), -1, mod), pow(n, -1, mod)
    want = []
    for i in range(n):
        acc = pts[n - 1]
        for j in range(n):
            acc = add(acc, mul(pts[j], pow(winv, i * j, mod) * ninv % mod))
        want.append(acc)
    assert kzg.to_lagrange_g2(_cat(tob, pts), log_n, curve=curve) == _cat(tob, want)


@pytest.mark.parametrize("curve", CURVES)
def test_to_lagrange_g2_against_the_trapdoor_and_aliasing(curve):
    """2^10: several blocks, every thread order of a stage; [L_i(tau)]2 by batch_scalar_mul of the Lagrange scalars"""
    from gnark_amd import fr, kzg, msm
    from gnark_amd._lib import DeviceBuffer
    _, _, tob, gen, pt, group = _g2(curve)
    mod, log_n = _mod(curve), 10
    n, w, t = 1 << log_n, _omega(curve, log_n), TAU % _mod(curve)
    mont = fr.fr_mont if curve == "bn254" else fr.bls_fr_mont
    c = (pow(t, n, mod) - 1) * pow(n, -1, mod) % mod
    lag = [c * pow(w, i, mod) * pow((t - pow(w, i, mod)) % mod, -1, mod) % mod for i in range(n)]
    want = msm.batch_scalar_mul(group, tob(gen), b"".join(mont(x) for x in lag), n)
    canon = _srs(curve, log_n).tau_g2
    assert len(canon) == pt * n
    assert kzg.to_lagrange_g2(canon, log_n, curve=curve) == want
    src = DeviceBuffer.from_host(canon)
    out = kzg.to_lagrange_g2(src, log_n, curve=curve, out_device=True)
    assert out.to_host() == want and src.to_host() == canon  # the input is left alone
    same = kzg.to_lagrange_g2(src, log_n, curve=curve, out=src)  # in == out
    assert same is src and src.to_host() == want


# ---------------------------------------------------------------- 9. the point checks
def _patched(srs, **parts):
    return dataclasses.replace(srs, **parts)


def _put(buf, index, pt):
    return buf[:index * len(pt)] + pt + buf[(index + 1) * len(pt):]


def test_check_points_bn254():
    import gnark_amd
    from gnark_amd import mpcsetup
    args, s = _cubic_csr("bn254"), _srs("bn254", 2)
    p = o.g1_mul(o.G1_GEN, 77)
    off_curve = o.g1_to_bytes((p[0], (p[1] + 1) % o.P))
    bad = _patched(s, alpha_tau_g1=_put(s.alpha_tau_g1, 3, off_curve))
    with pytest.raises(gnark_amd.GnarkAmdError) as e:
        mpcsetup.init_phase2(*args, bad)
    assert e.value.code == 1 and "alpha_tau_g1[3] is not on the curve" in str(e.value), str(e.value)
    mpcsetup.init_phase2(*args, bad, check_points=False).close()  # runs; the key is garbage
    with pytest.raises(gnark_amd.GnarkAmdError) as e:
        mpcsetup.init_phase2(*args, _patched(s, tau_g2=_put(s.tau_g2, 1, bytes(128))))
    assert e.value.code == 1 and "tau_g2[1] is the point at infinity" in str(e.value), str(e.value)
    mpcsetup.init_phase2(*args, s).close()  # the library still works


def test_check_points_bls12_381():
    import bls_pairing_ref as br
    import gnark_amd
    from gnark_amd import mpcsetup
    args, s = _cubic_csr("bls12-381"), _srs("bls12-381", 2)
    cases = [("tau_g1", 5, bls.g1_to_bytes(br.g1_off_curve(9)), "tau_g1[5] is not on the curve"),
             ("beta_tau_g1", 2, bls.g1_to_bytes(br.g1_outside_subgroup()), "beta_tau_g1[2] is not in the subgroup"),
             ("tau_g2", 3, bls.g2_to_bytes(br.twist_point_outside_subgroup(5)), "tau_g2[3] is not in the subgroup")]
    for name, index, pt, text in cases:
        bad = _patched(s, **{name: _put(getattr(s, name), index, pt)})
        with pytest.raises(gnark_amd.GnarkAmdError) as e:
            mpcsetup.init_phase2(*args, bad)
        assert e.value.code == 1 and text in str(e.value), str(e.value)
        mpcsetup.init_phase2(*args, bad, check_points=False).close()


def test_contribute_refusals():
    import gnark_amd
    from gnark_amd import groth16, mpcsetup
    from gnark_amd._lib import check, lib, ptr
    args = _cubic_csr("bn254")
    p2 = mpcsetup.init_phase2(*args, _srs("bn254", 2))
    with pytest.raises(gnark_amd.GnarkAmdError, match="delta is zero"):
        p2.contribute(0)
    p2.close()
    res = groth16.setup_device(*args, toxic_waste=_tw(D1, "bn254"))  # a key from the toxic waste takes none
    with pytest.raises(gnark_amd.GnarkAmdError, match="gg_groth16_setup_from_srs"):
        check(lib.gg_groth16_setup_contribute(res.handle, ptr(bytes([1]) + bytes(31))))
    res.close()

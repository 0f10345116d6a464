"""Groth16 Setup on the GPU (gnark_amd.groth16.setup, gg_groth16_setup;
backend/groth16/bn254/setup.go:85-337), bit-exact: a key is a deterministic
function of the R1CS and the toxic waste, so no tolerance exists.

Points are compared with the Python oracle's points where there are few, and
with msm.batch_scalar_mul of oracle SCALARS elsewhere (that function is pinned
to the oracle by tests/test_gpu_msm_batch.py)."""
import random
import types

import pytest

import bls12_381_oracle as bls
import bn254_bsb22 as bo
import bn254_oracle as o
import coracle
import r1cs_solver

pytestmark = pytest.mark.gpu

TW = dict(t=0x1DEA5EED1234567, alpha=0xA1FA0001, beta=0xBE7A0002, gamma=0x6A77A0004, delta=0xDE17A0003)
G1B, G2B = o.g1_to_bytes(o.G1_GEN), o.g2_to_bytes(o.G2_GEN)


def _tw(mod=o.R, **over):
    from gnark_amd import groth16
    d = dict(TW, **over)
    return groth16.ToxicWaste(d["t"] % mod, d["alpha"], d["beta"], d["gamma"], d["delta"])


def _cat1(pts):
    return b"".join(o.g1_to_bytes(p) for p in pts)


def _cat2(pts):
    return b"".join(o.g2_to_bytes(p) for p in pts)


def _frv(xs, mod=o.R):
    return b"".join(((x % mod) * (1 << 256) % mod).to_bytes(32, "little") for x in xs)


def _p1(scalars, curve="bn254"):
    from gnark_amd import msm
    if not scalars:
        return b""
    if curve == "bn254":
        return msm.batch_scalar_mul(msm.G1, G1B, _frv(scalars), len(scalars))
    return msm.batch_scalar_mul(msm.BLS12_381_G1, bls.g1_to_bytes(bls.G1_GEN), _frv(scalars, bls.R), len(scalars))


def _p2(scalars, curve="bn254"):
    from gnark_amd import msm
    if not scalars:
        return b""
    if curve == "bn254":
        return msm.batch_scalar_mul(msm.G2, G2B, _frv(scalars), len(scalars))
    return msm.batch_scalar_mul(msm.BLS12_381_G2, bls.g2_to_bytes(bls.G2_GEN), _frv(scalars, bls.R), len(scalars))


def _bitrev(i, log_n):
    return int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0


def _expected_scalars(A, B, C, nb_public, log_n, tw, mod):
    """the K and Z lines of setup.go:152-210 and the filtering of 212-237 on ints"""
    ginv, dinv = pow(tw.gamma, -1, mod), pow(tw.delta, -1, mod)
    k = [(a * tw.beta + b * tw.alpha + c) % mod for a, b, c in zip(A, B, C)]
    n = 1 << log_n
    zdt = (pow(tw.tau, n, mod) - 1) * dinv % mod
    Z = [zdt * pow(tw.tau, i, mod) % mod for i in range(n)]
    return dict(A=[a for a in A if a], B=[b for b in B if b], infA=bytes(int(a == 0) for a in A),
                infB=bytes(int(b == 0) for b in B), vkK=[x * ginv % mod for x in k[:nb_public]],
                pkK=[x * dinv % mod for x in k[nb_public:]], Z=[Z[_bitrev(i, log_n)] for i in range(n - 1)])


def _check_against_scalars(pk, vk, e, tw, curve="bn254"):
    assert bytes(pk.infinity_A) == e["infA"] and bytes(pk.infinity_B) == e["infB"]
    assert pk.g1_A == _p1(e["A"], curve)
    assert pk.g1_B == _p1(e["B"], curve)
    assert pk.g2_B == _p2(e["B"], curve)
    assert pk.g1_K == _p1(e["pkK"], curve)
    assert pk.g1_Z == _p1(e["Z"], curve)
    assert vk.K == _p1(e["vkK"], curve)
    assert pk.alpha1 + pk.beta1 + pk.delta1 == _p1([tw.alpha, tw.beta, tw.delta], curve)
    assert pk.beta2 + pk.delta2 + vk.gamma2 == _p2([tw.beta, tw.delta, tw.gamma], curve)
    assert (vk.alpha1, vk.beta1, vk.delta1, vk.beta2, vk.delta2) == \
        (pk.alpha1, pk.beta1, pk.delta1, pk.beta2, pk.delta2)


# ---------------------------------------------------------------- 1. cubic
def _cubic_bn254():
    from gnark_amd import groth16
    rcs = o.cubic_r1cs()
    tw = _tw()
    pk, vk = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, toxic_waste=tw)
    rp, rv = o.setup(rcs, o.ToxicWaste(tw.tau, tw.alpha, tw.beta, tw.gamma, tw.delta))
    assert pk.log_n == 2 and pk.nb_public == 2 and pk.k_wire_index is None and pk.commitment_keys is None
    assert pk.g1_A == _cat1(rp.g1_A) and pk.g1_B == _cat1(rp.g1_B) and pk.g2_B == _cat2(rp.g2_B)
    assert pk.g1_K == _cat1(rp.g1_K) and pk.g1_Z == _cat1(rp.g1_Z) and len(rp.g1_Z) == 3
    assert (pk.alpha1, pk.beta1, pk.delta1) == tuple(o.g1_to_bytes(p) for p in (rp.g1_alpha, rp.g1_beta, rp.g1_delta))
    assert (pk.beta2, pk.delta2) == (o.g2_to_bytes(rp.g2_beta), o.g2_to_bytes(rp.g2_delta))
    assert bytes(pk.infinity_A) == bytes(map(int, rp.infinity_A))
    assert bytes(pk.infinity_B) == bytes(map(int, rp.infinity_B))
    assert vk.K == _cat1(rv.g1_K) and vk.gamma2 == o.g2_to_bytes(rv.g2_gamma)
    assert (vk.alpha1, vk.beta2, vk.delta2) == (pk.alpha1, pk.beta2, pk.delta2)
    assert vk.commitment_key_g is None and list(vk.public_and_commitment_committed) == []
    return rcs, tw, pk, vk, rp


def test_cubic_bn254_every_field():
    _cubic_bn254()


def test_cubic_bls12_381():
    from gnark_amd import groth16
    rcs = o.cubic_r1cs()
    tw = _tw(bls.R)
    pk, vk = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, toxic_waste=tw,
                                      curve="bls12-381")
    ks = bls.groth16_setup_scalars(rcs.constraints, rcs.nb_wires, rcs.nb_public, 2, tw.tau, tw.alpha, tw.beta,
                                   tw.delta)
    g1 = lambda xs: b"".join(bls.g1_to_bytes(bls.g1_mul(bls.G1_GEN, x)) for x in xs)
    g2 = lambda xs: b"".join(bls.g2_to_bytes(bls.g2_mul(bls.G2_GEN, x)) for x in xs)
    assert pk.curve == "bls12-381" and pk.log_n == 2
    assert pk.g1_A == g1(ks["A"]) and pk.g1_B == g1(ks["B"]) and pk.g2_B == g2(ks["B"])
    assert pk.g1_K == g1(ks["K"]) and pk.g1_Z == g1(ks["Z"])
    assert bytes(pk.infinity_A) == bytes(ks["infA"]) and bytes(pk.infinity_B) == bytes(ks["infB"])
    ginv = pow(tw.gamma, -1, bls.R)
    vkk = [(ks["u"][i] * tw.beta + ks["v"][i] * tw.alpha + ks["w"][i]) * ginv % bls.R for i in range(rcs.nb_public)]
    assert vk.K == g1(vkk)
    assert pk.alpha1 + pk.beta1 + pk.delta1 == g1([tw.alpha, tw.beta, tw.delta])
    assert pk.beta2 + pk.delta2 + vk.gamma2 == g2([tw.beta, tw.delta, tw.gamma])


# ---------------------------------------------------------------- 2. random systems
@pytest.mark.parametrize("curve,seed", [("bn254", 1), ("bn254", 2), ("bls12-381", 3)])
def test_random_systems(curve, seed):
    from gnark_amd import groth16
    mod = o.R if curve == "bn254" else bls.R
    rng = random.Random(8800 + seed)
    nb_public, nb_secret, n_int = 3, 5, 700 + seed  # domain 1024, ~710 wires: several 256-thread blocks
    cons = r1cs_solver.random_circuit(rng, nb_public, nb_secret, n_int, R=mod)
    nw = nb_public + nb_secret + n_int
    tw = _tw(mod)
    pk, vk = groth16.setup_from_terms(nb_public, nw, cons, toxic_waste=tw, curve=curve)
    assert pk.log_n == 10
    if curve == "bn254":
        rcs = o.R1CS(nb_public, nb_secret, n_int, cons)
        A, B, C = o.setup_abc(rcs, o.Domain(len(cons)), o.ToxicWaste(tw.tau, tw.alpha, tw.beta, tw.gamma, tw.delta))
    else:
        ks = bls.groth16_setup_scalars(cons, nw, nb_public, 10, tw.tau, tw.alpha, tw.beta, tw.delta)
        A, B, C = ks["u"], ks["v"], ks["w"]
    _check_against_scalars(pk, vk, _expected_scalars(A, B, C, nb_public, 10, tw, mod), tw, curve)


# ---------------------------------------------------------------- 3. hand-built edges
def test_edge_system():
    """n_constraints = 512 = the domain (the j = n - 1 term); raw CSR with the
    coefficient table [0, 1, 2, -1, k]: ids 0..3 go through the table like any other."""
    from gnark_amd import groth16
    ncons, nb_public = 512, 2
    # the chunk size comes from a tiny setup's info
    res = groth16.setup_device(2, 5, [0, 1, 2, 3], [2, 2, 3], [1, 1, 1], [0, 1], toxic_waste=_tw())
    C = res.acc_chunk
    res.close()
    assert C >= 2
    table = [0, 1, 2, o.R - 1, 0x1234567890ABCDEF]
    PM, DUP, DM1, DC, DP1, DSQ, ZERO_ID, FREE = 2, 3, 4, 5, 6, 7, 8, 9
    nw = FREE + 20
    assert C * C + 1 <= 3 * ncons
    sides = [[[(0, 1)], [], []] for _ in range(ncons)]  # wire 0, coefficient 1, in L of EVERY constraint
    for j in range(ncons):
        sides[j][2].append((FREE + j % 20, 1))          # wires absent from every R
    sides[5][0] += [(PM, 1), (PM, 3)]                   # +1 and -1 in one constraint: A[PM] = 0 by value
    sides[7][1] += [(DUP, 2), (DUP, 3)]                 # twice in one side, ids 2 and 3
    sides[9][1] += [(ZERO_ID, 0)]                       # id 0: B[ZERO_ID] = 0 although the wire occurs
    for j in range(C - 1):
        sides[j][2].append((DM1, 4))                    # degree chunk - 1
    for j in range(C):
        sides[100 + j][2].append((DC, 4))               # degree chunk
    for j in range(C + 1):
        sides[200 + j][1].append((DP1, 4))              # degree chunk + 1
    left = C * C + 1                                    # degree chunk^2 + 1: up to three per constraint
    for j in range(ncons):
        for _ in range(min(3, left)):
            sides[j][1].append((DSQ, 4))
            left -= 1
    assert left == 0
    off, wires, cids = [0], [], []
    for s3 in sides:
        for side in s3:
            wires += [w for w, _ in side]
            cids += [c for _, c in side]
            off.append(len(wires))
    tw = _tw()
    pk, vk = groth16.setup(nb_public, nw, off, wires, cids, table, toxic_waste=tw)
    assert pk.log_n == 9
    # A[0] = sum_j L_j(tau) = 1: the first G1.A point is the generator (needs no oracle)
    assert pk.g1_A[:64] == G1B
    assert pk.infinity_A[0] == 0 and pk.infinity_A[PM] == 1 and pk.infinity_B[DUP] == 0
    assert pk.infinity_B[ZERO_ID] == 1 and all(pk.infinity_B[FREE:])
    rcs = o.R1CS(nb_public, 0, nw - nb_public, [tuple([(w, table[c]) for w, c in side] for side in s3)
                                                for s3 in sides])
    A, B, Cc = o.setup_abc(rcs, o.Domain(ncons), o.ToxicWaste(tw.tau, tw.alpha, tw.beta, tw.gamma, tw.delta))
    assert A[0] == 1 and A[PM] == 0
    _check_against_scalars(pk, vk, _expected_scalars(A, B, Cc, nb_public, 9, tw, o.R), tw)


# ---------------------------------------------------------------- 4. MiMC shape, C oracle
@pytest.mark.parametrize("log_n", [12, 16])
def test_mimc_against_c_oracle(log_n):
    from gnark_amd import groth16, msm
    from test_gpu_solver import mimc_csr
    chains, rounds = 1 << (log_n - 8), 85
    m = mimc_csr(chains, rounds, 1)
    cr = coracle.MimcR1CS(chains, rounds, 1)
    assert (cr.ncons, cr.nw, cr.nb_public) == (m["ncons"], m["nw"], m["nb_public"])
    tw = _tw()
    f = lambda v: o.fr_to_bytes(v % o.R)
    ks = cr.key_scalars(log_n, f(tw.tau), f(tw.alpha), f(tw.beta), f(tw.delta))
    cr.close()
    res = groth16.setup_device(m["nb_public"], m["nw"], m["off"], m["wires"], m["coef"], m["table"], toxic_waste=tw)
    if log_n == 16:  # wire 0 has 256 * 85 = 21,760 O-side terms: more than two rounds of the reduction
        assert 21760 > res.acc_chunk ** 2 and res.acc_launches >= 3
    res.close()
    pk, vk = groth16.setup(m["nb_public"], m["nw"], m["off"], m["wires"], m["coef"], m["table"], toxic_waste=tw)
    assert pk.log_n == log_n
    assert bytes(pk.infinity_A) == ks["infA"] and bytes(pk.infinity_B) == ks["infB"]
    p1 = lambda sc: msm.batch_scalar_mul(msm.G1, G1B, sc, len(sc) // 32)
    assert pk.g1_A == p1(ks["A"]) and pk.g1_B == p1(ks["B"])
    assert pk.g1_K == p1(ks["K"]) and pk.g1_Z == p1(ks["Z"])
    assert pk.g2_B == msm.batch_scalar_mul(msm.G2, G2B, ks["B"], len(ks["B"]) // 32)


# ---------------------------------------------------------------- 5. commitments
@pytest.mark.parametrize("nc", [1, 2])
def test_commitments(nc):
    from gnark_amd import groth16
    rcs, cinfo = bo.bsb22_test_circuit(nc)
    tw = _tw()
    rp, rv = bo.setup_bsb22(rcs, o.ToxicWaste(tw.tau, tw.alpha, tw.beta, tw.gamma, tw.delta), cinfo,
                            sigma=424242, g_scalar=77)
    com = [(c.commitment_index, c.private_committed, c.public_committed) for c in cinfo]
    pk, vk = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, commitments=com,
                                      toxic_waste=tw, pedersen=(424242, 77))
    assert pk.g1_K == _cat1(rp.g1_K) and list(pk.k_wire_index) == rp.k_wire_index
    assert vk.K == _cat1(rv.g1_K) and len(rv.g1_K) == rcs.nb_public + nc
    assert len(pk.commitment_keys) == nc
    for j in range(nc):
        assert pk.commitment_keys[j].basis == _cat1(rp.commitment_keys[j].basis)
        assert pk.commitment_keys[j].basis_exp_sigma == _cat1(rp.commitment_keys[j].basis_exp_sigma)
    assert vk.commitment_key_g == o.g2_to_bytes(rv.commitment_key.g)
    assert vk.commitment_key_g_root_sigma_neg == o.g2_to_bytes(rv.commitment_key.g_root_sigma_neg)
    assert [list(x) for x in vk.public_and_commitment_committed] == rv.public_committed
    assert pk.g1_A == _cat1(rp.g1_A) and pk.g2_B == _cat2(rp.g2_B) and pk.g1_Z == _cat1(rp.g1_Z)
    dev = groth16.ProvingKey(pk)  # goes straight into the device key, Pedersen bases included
    assert len(dev.commitment_keys) == nc
    dev.close()


# ---------------------------------------------------------------- 6. end to end
def _oracle_vk(vk):
    k = [o.g1_from_bytes(vk.K[i:i + 64]) for i in range(0, len(vk.K), 64)]
    return types.SimpleNamespace(g1_alpha=o.g1_from_bytes(vk.alpha1), g2_beta=o.g2_from_bytes(vk.beta2),
                                 g2_gamma=o.g2_from_bytes(vk.gamma2), g2_delta=o.g2_from_bytes(vk.delta2), g1_K=k)


def _prove(rcs, pk, witness, r, s):
    from gnark_amd import backend, groth16, solver
    dev = groth16.ProvingKey(pk)
    sys_ = solver.R1CS.from_terms(rcs.nb_public, rcs.nb_secret, rcs.nb_wires, rcs.constraints)
    pr = groth16.prove(dev, sys_.solve(witness), backend.with_amd_acceleration(), r=o.fr_to_bytes(r),
                       s=o.fr_to_bytes(s))
    sys_.close()
    dev.close()
    return pr


def test_end_to_end_cubic():
    rcs, tw, pk, vk, rp = _cubic_bn254()
    r, s = 0x5EED0001, 0x5EED0002
    pr = _prove(rcs, pk, [35, 3], r, s)
    ref = o.prove(rcs, rp, o.cubic_witness(3, 35), r, s)
    assert (pr.Ar, pr.Bs, pr.Krs) == (o.g1_to_bytes(ref.Ar), o.g2_to_bytes(ref.Bs), o.g1_to_bytes(ref.Krs))
    proof = o.Proof(o.g1_from_bytes(pr.Ar), o.g2_from_bytes(pr.Bs), o.g1_from_bytes(pr.Krs))
    assert o.verify(proof, _oracle_vk(vk), [35])
    assert not o.verify(proof, _oracle_vk(vk), [36])


def test_end_to_end_mimc_chain():
    from gnark_amd import groth16
    rcs = o.mimc_chain_r1cs(2, 5)
    pk, vk = groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints)  # sampled toxic waste
    pr = _prove(rcs, pk, [11, 22], 7, 9)
    proof = o.Proof(o.g1_from_bytes(pr.Ar), o.g2_from_bytes(pr.Bs), o.g1_from_bytes(pr.Krs))
    assert o.verify(proof, _oracle_vk(vk), [])
    bad = o.Proof(proof.Ar, proof.Bs, o.g1_add(proof.Krs, o.G1_GEN))
    assert not o.verify(bad, _oracle_vk(vk), [])


# ---------------------------------------------------------------- 7. errors
def test_errors_then_the_library_still_works():
    import gnark_amd
    from gnark_amd import fr, groth16
    rcs = o.cubic_r1cs()

    def refused(text, **kw):
        args = dict(toxic_waste=_tw())
        args.update(kw)
        with pytest.raises(gnark_amd.GnarkAmdError) as e:
            groth16.setup_from_terms(rcs.nb_public, rcs.nb_wires, rcs.constraints, **args)
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    refused("tau is in the domain", toxic_waste=_tw(t=pow(fr.domain_generator(2), 3, o.R)))
    refused("delta is zero", toxic_waste=_tw(delta=0))
    with pytest.raises(gnark_amd.GnarkAmdError) as e:   # a term wire >= n_wires
        groth16.setup(2, 5, [0, 1, 2, 3], [2, 5, 3], [0, 0, 0], [1], toxic_waste=_tw())
    assert e.value.code == 1 and "wire id 5 out of range" in str(e.value)
    with pytest.raises(gnark_amd.GnarkAmdError) as e:   # a coefficient id >= n_coeffs
        groth16.setup(2, 5, [0, 1, 2, 3], [2, 4, 3], [0, 1, 0], [1], toxic_waste=_tw())
    assert e.value.code == 1 and "coefficient id 1 out of range" in str(e.value)
    _cubic_bn254()

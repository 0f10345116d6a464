"""PlonK Setup, the parts that need no GPU: the reference restatement
(plonk_setup_ref.py) against hand-worked values and the closed form of the
Lagrange SRS, gg_plonk_setup_sizes, and every refusal of
gg_kzg_to_lagrange_g1 / gg_plonk_setup -- all of them are decided on the host
before the first device call, so they answer on a machine without a GPU."""
import ctypes

import numpy as np
import pytest

import plonk_prover_oracle as po
import plonk_setup_ref as ref

CURVES = ("bls12-381", "bn254")


# ------------------------------------------------------------ the reference
def test_ref_permutation_hand_worked():
    """nb_public = 1, two constraints (a, b, c) = (1, 0, 2), (2, 2, 1), n = 4:
         row      L  R  O
         0 (pub)  0  0  0      R, O of a public row: unfilled, wire 0
         1        1  0  2
         2        2  2  1
         3 (pad)  0  0  0      padding: wire 0 three times
    positions by wire: 0 -> 0, 3, 4, 5, 7, 8, 11; 1 -> 1, 10; 2 -> 2, 6, 9.
    Every position links to the one before it in its list, the first to the last."""
    cons = [(1, 0, 2, 0, 0, 0, 0, 0), (2, 2, 1, 0, 0, 0, 0, 0)]
    assert ref.build_lro(cons, 1, 4) == [0, 1, 2, 0, 0, 0, 2, 0, 0, 2, 1, 0]
    want = [None] * 12
    for cyc in ([0, 3, 4, 5, 7, 8, 11], [1, 10], [2, 6, 9]):
        for k, pos in enumerate(cyc):
            want[pos] = cyc[k - 1]  # k = 0: the last
    assert ref.build_permutation(cons, 1, 3) == want
    assert want[0] == 11 and want[3] == 0 and want[11] == 8  # the wire-0 padding cycle


@pytest.mark.parametrize("seed", range(4))
def test_ref_permutation_is_a_permutation_preserving_lro(seed):
    import random
    import scs_solver as ss
    rng = random.Random(seed)
    nbp = seed % 3
    cons, _flags, nw = ss.random_circuit(rng, po.BLS12_381.R, nbp, 3, 37 + seed)
    cons = ss.fill_assertions(po.BLS12_381.R, cons, [5, 6, 7, 8, 9])
    n = ref.next_pow2(len(cons) + nbp)
    perm = ref.build_permutation(cons, nbp, nw)
    lro = ref.build_lro(cons, nbp, n)
    assert sorted(perm) == list(range(3 * n))
    assert all(lro[perm[i]] == lro[i] for i in range(3 * n))
    # maximal cycles: following perm from any position of a wire visits all its positions
    for start in (0, n, 3 * n - 1):
        seen, p = set(), start
        while p not in seen:
            seen.add(p)
            p = perm[p]
        assert seen == {i for i in range(3 * n) if lro[i] == lro[start]}


def test_ref_domains():
    assert ref.init_domains(2, 0) == (2, 16)
    assert ref.init_domains(2, 3) == (8, 64)    # sizeSystem 5: n = 8 but the big domain is 8 * 5 -> 64
    assert ref.init_domains(6, 0) == (8, 32)
    assert ref.init_domains(61, 3) == (64, 256)
    assert ref.init_domains(65, 0) == (128, 512)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [4, 8])
def test_ref_to_lagrange_equals_closed_form(curve, n):
    cv = po.curve(curve)
    tau = 0x1234567 + n
    w = cv.omega(n)
    srs = [cv.mul(cv.G1, pow(tau, j, cv.R)) for j in range(n)]
    got = ref.to_lagrange_ref(cv, srs, w)
    want = [cv.mul(cv.G1, c) for c in ref.lagrange_at(cv.R, n, w, tau)]
    assert got == want


# ------------------------------------------------------------ gg_plonk_setup_sizes
def _sizes(n_cons, nb_public):
    from gnark_amd import plonk_prover as pp
    return pp.setup_sizes(n_cons, nb_public)


def test_sizes_follow_gnark():
    from gnark_amd._lib import GnarkAmdError
    for size_system in (0, 1):
        with pytest.raises(GnarkAmdError) as e:
            _sizes(size_system, 0)
        assert e.value.code == 1 and "sizeSystem" in str(e.value)
    assert _sizes(2, 0) == (1, 4)
    assert _sizes(3, 0) == (2, 5)
    assert _sizes(2, 3) == (3, 6)     # sizeSystem 5: n = 8, big = 8 n
    assert _sizes(5, 0) == (3, 6)
    assert _sizes(3, 3) == (3, 5)     # sizeSystem 6: big = 4 n
    for k in (3, 6, 10, 20):
        assert _sizes(1 << k, 0) == (k, k + 2)
        assert _sizes((1 << k) - 2, 3) == (k + 1, k + 3)  # 2^k + 1
    for nc, nbp in ((2, 0), (2, 3), (3, 3), (64, 0), (62, 3), (3000, 3)):
        n, big = ref.init_domains(nc, nbp)
        assert _sizes(nc, nbp) == (n.bit_length() - 1, big.bit_length() - 1)
    with pytest.raises(GnarkAmdError) as e:
        _sizes((1 << 27) + 1, 0)
    assert e.value.code == 1 and "log_n" in str(e.value)


# ------------------------------------------------------------ refusals of gg_kzg_to_lagrange_g1
def _ec(curve, log_n, omega, pts=b"\0" * 192, out=None, null=None):
    from gnark_amd import fr
    from gnark_amd._lib import GG_CURVE_BLS12_381, GG_CURVE_BN254, lib, ptr
    cid = {"bls12-381": GG_CURVE_BLS12_381, "bn254": GG_CURVE_BN254}.get(curve, curve)
    mont = fr.fr_mont if curve == "bn254" else fr.bls_fr_mont
    out = bytearray(len(pts)) if out is None else out
    args = [ptr(mont(omega)), ptr(pts), ptr(out)]
    if null is not None:
        args[null] = None
    rc = lib.gg_kzg_to_lagrange_g1(cid, log_n, args[0], args[1], 0, args[2], 0, None)
    return rc, lib.gg_last_error().decode()


@pytest.mark.parametrize("curve", CURVES)
def test_ecntt_refusals(curve):
    cv = po.curve(curve)
    for null, name in ((0, "omega_mont"), (1, "g1_in"), (2, "g1_out")):
        rc, msg = _ec(curve, 1, cv.omega(2), null=null)
        assert rc == 1 and name in msg
    for log_n in (0, -1, 28):
        rc, msg = _ec(curve, log_n, 1)
        assert rc == 1 and "log_n" in msg
    rc, msg = _ec(curve, 3, cv.omega(4))       # order 4, not 8
    assert rc == 1 and "omega" in msg
    rc, msg = _ec(curve, 2, cv.omega(8))       # order 8, not 4
    assert rc == 1 and "omega" in msg
    rc, msg = _ec(curve, 1, 1)
    assert rc == 1 and "omega" in msg
    rc, msg = _ec(7, 1, cv.omega(2))
    assert rc == 1 and "curve" in msg


# ------------------------------------------------------------ refusals of gg_plonk_setup
class _Sys:
    """A valid call of gg_plonk_setup (sizeSystem 5, n = 8) whose fields the cases break one at a time."""

    def __init__(self, curve):
        from gnark_amd import fr
        self.curve = curve
        self.cv = po.curve(curve)
        self.mont = fr.fr_mont if curve == "bn254" else fr.bls_fr_mont
        self.pt = 64 if curve == "bn254" else 96
        self.n_wires, self.nb_public = 6, 1
        self.wires = [0, 1, 2, 2, 3, 4, 4, 0, 5, 1, 1, 1]
        self.qidx = [0, 1, 2, 3, 0] * 4
        self.n_coeffs = 4
        self.committed, self.cmt_idx = [[0, 2]], [3]
        self.omega = self.cv.omega(8)
        self.n_kzg = 11
        self.curve_id = None

    def call(self):
        from gnark_amd._lib import GG_CURVE_BLS12_381, GG_CURVE_BN254, lib, ptr
        cid = self.curve_id if self.curve_id is not None else \
            (GG_CURVE_BN254 if self.curve == "bn254" else GG_CURVE_BLS12_381)
        wires = np.array(self.wires, np.uint32)
        qidx = np.array(self.qidx, np.uint32)
        coeffs = b"".join(self.mont(k) for k in range(max(1, self.n_coeffs)))
        nc = len(self.committed)
        off = np.zeros(nc + 1, np.uint32)
        off[1:] = np.cumsum([len(c) for c in self.committed])
        flat = np.array([k for c in self.committed for k in c], np.uint32)
        idx = (ctypes.c_uint64 * max(1, nc))(*self.cmt_idx)
        kzg = bytes(self.pt * max(1, self.n_kzg))
        h = ctypes.c_void_p()
        rc = lib.gg_plonk_setup(cid, self.n_wires, len(self.wires) // 3, self.nb_public, ptr(wires), ptr(qidx),
                                ptr(coeffs), self.n_coeffs, nc, ptr(off), ptr(flat), idx, ptr(self.mont(self.omega)),
                                ptr(self.mont(self.cv.fr_gen)), ptr(kzg), self.n_kzg, None, ctypes.byref(h))
        assert h.value is None
        return rc, lib.gg_last_error().decode()


def _break(s, what):
    if what == "n_wires":
        s.n_wires = 0
    elif what == "wire":
        s.wires[7] = 6
    elif what == "coefficient":
        s.qidx[11] = 4
    elif what == "committed":
        s.committed = [[0, 4]]
    elif what == "commitment":
        s.cmt_idx = [7]          # nb_public + 7 = n
    elif what == "n_kzg":
        s.n_kzg = 10             # n + 2
    elif what == "n_cmt":
        s.committed, s.cmt_idx = [[0]] * 9, [0] * 9
    elif what == "omega":
        s.omega = s.cv.omega(16)
    elif what == "sizeSystem":
        s.wires, s.qidx, s.nb_public, s.committed, s.cmt_idx = [0, 0, 0], [0] * 5, 0, [], []
    elif what == "curve":
        s.curve_id = 5


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("what", ["n_wires", "wire", "coefficient", "committed", "commitment", "n_kzg", "n_cmt",
                                  "omega", "sizeSystem", "curve"])
def test_setup_refusals_name_the_offender(curve, what):
    s = _Sys(curve)
    _break(s, what)
    rc, msg = s.call()
    assert rc == 1, (rc, msg)
    assert what in msg, msg
    if what == "wire":
        assert "constraint 2" in msg and "wire id 6" in msg
    if what == "coefficient":
        assert "constraint 2" in msg and "coefficient id 4" in msg
    if what == "committed":
        assert "index 4" in msg


def test_setup_log_n_above_27_is_refused_by_size():
    """log_n > 27 is decided from the counts alone: no array is read before it."""
    from gnark_amd._lib import lib
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.gg_plonk_setup_sizes((1 << 27) - 2, 3, ctypes.byref(a), ctypes.byref(b)) == 1
    assert "log_n" in lib.gg_last_error().decode()
    h = ctypes.c_void_p()
    one = bytes(96)
    rc = lib.gg_plonk_setup(1, 5, (1 << 27) + 1, 0, None, None, one, 1, 0, None, None, None, one, one, one, 1 << 28,
                            None, ctypes.byref(h))
    assert rc == 1 and "log_n" in lib.gg_last_error().decode()

"""Groth16 keys from a powers-of-tau SRS, the parts that need no GPU: the three
exports and their declarations, and every refusal that gg_groth16_setup_from_srs,
gg_groth16_setup_contribute and gg_kzg_to_lagrange_g2 decide before any device
call (code GG_ERR_INVALID_ARG, the message naming the offender)."""
import ctypes
import os
import re

import pytest

SYMBOLS = ["gg_kzg_to_lagrange_g2", "gg_groth16_setup_from_srs", "gg_groth16_setup_contribute"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn254", "bls12-381")


def test_the_three_symbols_are_exported_and_declared():
    from gnark_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and getattr(_lib.lib, name) is not None, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    from gnark_amd import mpcsetup
    assert mpcsetup.TIMINGS[:9] == ["transpose", "lagrange", "accumulate", "kz", "g1", "g2", "accumulate_kernels",
                                    "accumulate_threads", "terms"]
    assert len(mpcsetup.TIMINGS) == _lib.GG_SETUP_TIMING_SLOTS
    assert "#define GG_SETUP_TIMING_SLOTS %d" % _lib.GG_SETUP_TIMING_SLOTS in header


def _srs(curve, n):
    """zero bytes of the right sizes: a refused call never reads them"""
    from gnark_amd import mpcsetup
    g1 = 64 if curve == "bn254" else 96
    return mpcsetup.Phase1Srs(bytes(g1 * (2 * n - 1)), bytes(g1 * n), bytes(g1 * n), bytes(2 * g1 * n), bytes(2 * g1),
                              n=n, curve=curve)


# four constraints over six wires: the domain is 4
CSR = dict(term_off=list(range(13)), term_wire=[1, 2, 3] * 4, term_coeff=[0] * 12, coeffs=[1])


def _refused(text, curve, n, **over):
    import gnark_amd
    from gnark_amd import mpcsetup
    a = dict(CSR, **over)
    with pytest.raises(gnark_amd.GnarkAmdError) as e:
        mpcsetup.init_phase2(2, 6, a["term_off"], a["term_wire"], a["term_coeff"], a["coeffs"], _srs(curve, n))
    assert e.value.code == 1 and text in str(e.value), str(e.value)


@pytest.mark.parametrize("curve", CURVES)
def test_from_srs_refusals(curve):
    _refused("srs_n 12 is not a power of two", curve, 12)  # 3 * 2^2
    _refused("srs_n 96 is not a power of two", curve, 96)  # 3 * 2^5
    _refused("srs_n 2 is below the domain of n_constraints (4)", curve, 2)
    _refused("wire id 6 out of range", curve, 4, term_wire=[1, 2, 3] * 3 + [1, 6, 3])
    _refused("coefficient id 1 out of range", curve, 4, term_coeff=[0] * 11 + [1])


def _raw_from_srs(curve, omega_int, null=None):
    """the C entry point with a chosen omega (init_phase2 always passes the domain's own)"""
    import numpy as np
    from gnark_amd import fr
    from gnark_amd._lib import GG_CURVE_BLS12_381, GG_CURVE_BN254, lib, ptr
    bn = curve == "bn254"
    mont = fr.fr_mont if bn else fr.bls_fr_mont
    s = _srs(curve, 4)
    g1, g2 = fr.generators(curve)
    off = np.asarray(CSR["term_off"], dtype=np.uint32)
    wire = np.asarray(CSR["term_wire"], dtype=np.uint32)
    cid = np.asarray(CSR["term_coeff"], dtype=np.uint32)
    parts = dict(tau_g1=s.tau_g1, alpha_tau_g1=s.alpha_tau_g1, beta_tau_g1=s.beta_tau_g1, tau_g2=s.tau_g2,
                 beta_g2=s.beta_g2)
    if null:
        parts[null] = None
    flat = []
    for p in parts.values():
        flat += [ptr(p), 0]
    h = ctypes.c_void_p()
    rc = lib.gg_groth16_setup_from_srs(GG_CURVE_BN254 if bn else GG_CURVE_BLS12_381, 6, 4, 2, ptr(off), ptr(wire),
                                       ptr(cid), ptr(mont(1)), 1, *flat, 4, 1, ptr(mont(omega_int)), ptr(g1), ptr(g2),
                                       ctypes.byref(h))
    return rc, (lib.gg_last_error() or b"").decode(), h.value


@pytest.mark.parametrize("curve", CURVES)
def test_from_srs_refuses_a_bad_omega_and_null_arguments(curve):
    from gnark_amd import fr
    gen = fr.domain_generator if curve == "bn254" else fr.bls_domain_generator
    for w in (gen(3), gen(1), 1):  # order 8, 2 and 1: none generates the domain of 4
        rc, msg, h = _raw_from_srs(curve, w)
        assert rc == 1 and "omega is not a generator of the domain" in msg and not h, msg
    for name in ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2", "beta_g2"):
        rc, msg, h = _raw_from_srs(curve, gen(2), null=name)
        assert rc == 1 and msg.endswith("null argument: " + name) and not h, msg


def test_contribute_refusals():
    from gnark_amd._lib import lib, ptr
    one = bytes([1]) + bytes(31)
    assert lib.gg_groth16_setup_contribute(None, ptr(one)) == 1
    assert b"null handle" in lib.gg_last_error()
    assert lib.gg_groth16_setup_contribute(None, ptr(bytes(32))) == 1  # delta = 0, before the handle is looked at
    assert b"delta is zero" in lib.gg_last_error()
    assert lib.gg_groth16_setup_contribute(None, None) == 1
    assert b"null argument: delta" in lib.gg_last_error()


@pytest.mark.parametrize("curve", CURVES)
def test_to_lagrange_g2_refusals(curve):
    """the contract of gg_kzg_to_lagrange_g1: refused before any device call"""
    import gnark_amd
    from gnark_amd import fr, kzg
    from gnark_amd._lib import GG_CURVE_BLS12_381, GG_CURVE_BN254, lib, ptr
    bn = curve == "bn254"
    cid, pt = (GG_CURVE_BN254, 128) if bn else (GG_CURVE_BLS12_381, 192)
    mont, gen = (fr.fr_mont, fr.domain_generator) if bn else (fr.bls_fr_mont, fr.bls_domain_generator)
    pts = bytes(pt * 8)
    with pytest.raises(gnark_amd.GnarkAmdError) as e:
        kzg.to_lagrange_g2(pts, 3, curve=curve, omega=gen(2))  # order 4, not 8
    assert e.value.code == 1 and "omega is not of exact order n = 2^3" in str(e.value)
    out = bytearray(pt * 8)
    w = mont(gen(3))
    for args, text in [((cid, 3, None, ptr(pts), 0, ptr(out), 0, None), "null argument: omega_mont"),
                       ((cid, 3, ptr(w), None, 0, ptr(out), 0, None), "null argument: g2_in"),
                       ((cid, 3, ptr(w), ptr(pts), 0, None, 0, None), "null argument: g2_out"),
                       ((cid, 0, ptr(w), ptr(pts), 0, ptr(out), 0, None), "log_n 0 out of range"),
                       ((cid, 28, ptr(w), ptr(pts), 0, ptr(out), 0, None), "log_n 28 out of range"),
                       ((7, 3, ptr(w), ptr(pts), 0, ptr(out), 0, None), "unknown curve 7")]:
        assert lib.gg_kzg_to_lagrange_g2(*args) == 1
        assert text in lib.gg_last_error().decode(), lib.gg_last_error()

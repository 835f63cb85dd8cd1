"""Traced ray differentials of spectral records without a GPU: the C-ABI declares and exports the call, the arithmetic of
csrc/differentials_spectral.hpp (compiled for the host) agrees with f64 central differences of the numpy restatement
(differentials_spectral_ref.py), reproduces the d-line tangents bit for bit where the wavelength changes nothing, the feature is
needed on the shipped TESSAR, the wavelength tangent has the sign and the size physics asks for, and the gfx950 kernels keep their
budget.

Rays: ~10 k passing rays per lens, wavelengths uniform in [400, 700] nm plus the eight of spectral_ref.WAVES.  The measured
figures are in test_wavelength_tangent_ratio_to_its_own_size.
"""
import ctypes
import re

import numpy as np
import pytest

from zoic_amd import _capi

import differentials_ref as dref
import differentials_spectral_ref as sref
import host_drivers
from device_cases import bits_f32 as _bits
from differentials_spectral_ref import lens_rays as _rays, passes as _passes, ray_wavelengths as _wavelengths, tables
from host_drivers import run_differentials_spectral as run_driver
from library_facts import header_text, kernel_resources
from spectral_ref import LAMBDA_D32, SINGLET, WAVES

NAME = "zoic_ray_differentials_spectral_device"
F32 = np.float32


def test_abi_declares_and_exports_the_call():
    text = header_text()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert NAME in _capi.SYMBOLS
    assert len(_capi.SYMBOLS[NAME][1]) == 12
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    assert hasattr(_capi.load(), NAME)
    assert _capi.load().zoic_abi_version() == 5 and _capi.ABI_VERSION == 5


@pytest.fixture(scope="module")
def driver():
    return host_drivers.differentials_spectral()


def test_per_ray_interface_is_the_d_line_restatement():
    """sref.interface is differentials_ref._interface, bit for bit, for one eta"""
    rs = np.random.RandomState(2)
    o = rs.uniform(-1, 1, (500, 3))
    d = rs.uniform(-0.3, 0.3, (500, 3)) + [0, 0, -1]
    for eta in (1.0, 1.6, 1 / 1.7):
        a = dref._interface(o, d, -30.0, 900.0, 1.0, eta)
        b = sref.interface(o, d, -30.0, 900.0, 1.0, np.full(500, eta))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


CASES = [("C2", None), ("C3", 50.0), ("C5", None)]
_MEASURED = {}


def _measure(cfg, abbe, driver, oracle_lib):
    """the host build against the f64 central differences on one lens's rays: the figures the two tests below assert on"""
    if cfg in _MEASURED:
        return _MEASURED[cfg]
    p, info, disp, surf, hs = tables(cfg, abbe)
    assert disp["cauchy_b"].any()
    o, d = _rays(cfg, oracle_lib)
    lam = _wavelengths(len(o))
    ok = _passes(surf, sref.cauchy_eta(disp, lam), o, d)   # the d-line's passing rays that also pass at their wavelength
    assert ok.mean() > 0.98, (cfg, float(ok.mean()))
    o, d, lam = o[ok], d[ok], lam[ok]
    assert len(o) >= 5000 and np.isin(WAVES, lam).sum() >= 6
    out, chroma, prim = run_driver(driver, 2, surf, disp, hs, lam, o, d)
    out12, chroma0, _ = run_driver(driver, 1, surf, disp, hs, lam, o, d)
    assert np.array_equal(_bits(out), _bits(out12)) and not _bits(chroma0).any()   # the third tangent changes nothing else
    assert np.isfinite(out).all() and np.isfinite(chroma).all()
    ro, rd, _ = sref.trace(surf, sref.cauchy_eta(disp, lam), o, d)
    assert np.allclose(prim[:, 0:3], -ro, rtol=1e-4, atol=1e-4) and np.allclose(prim[:, 3:6], -rd, rtol=1e-4, atol=1e-5)
    e = dref.rel_err(out, sref.jacobian_fd(surf, disp, lam, hs, o, d))
    fd = sref.wavelength_fd(surf, disp, lam, o, d, h=0.05)
    el = sref.rel_err_floor(chroma, fd)
    # halving the step moves the central difference by less than the tightest bound it is used with
    step = sref.rel_err_floor(sref.wavelength_fd(surf, disp, lam, o, d, h=0.025), fd)
    # the same error against the sum of the interfaces' contributions (what f32 can hold it to: sref.wavelength_contributions)
    part = sref.wavelength_contributions(surf, disp, lam, o, d)
    diff = np.linalg.norm((chroma.astype(np.float64) - fd).reshape(-1, 2, 3), axis=2)
    ec = diff / part
    m = dict(s_med=float(np.median(e)), s_tail=float(np.percentile(e, 99.9)), l_med=float(np.median(el)),
             l_tail=float(np.percentile(el, 99.9)), c_med=float(np.median(ec)), c_tail=float(np.percentile(ec, 99.9)),
             step=float(np.percentile(step, 99.9)),
             cancel=float(np.median(part[:, 1] / np.linalg.norm(fd[:, 3:6], axis=1))))
    print(cfg, " ".join("%s %.2e" % kv for kv in m.items()))
    _MEASURED[cfg] = m
    return m


@pytest.mark.parametrize("cfg,abbe", CASES, ids=["C2", "C3-V50", "C5"])
def test_tangents_match_finite_differences(cfg, abbe, driver, oracle_lib):
    """Screen tangents: the project's bounds for this arithmetic (median <= 1e-5, 99.9th percentile <= 1e-3, no ray left out).
    Wavelength tangent: its error, measured against the SUM of the magnitudes of the interfaces' contributions (the f64 reference's:
    sref.wavelength_contributions), is at most 4 x the screen tangents' own figures on the same rays: the arithmetic is the same
    transfer terms plus one source term per interface, so a larger gap is a wrong term (a check that does not depend on how much the
    contributions cancel; test_wavelength_tangent_ratio_to_its_own_size has the one against the tangent's own size)."""
    m = _measure(cfg, abbe, driver, oracle_lib)
    assert m["step"] < 4 * m["s_med"], m
    assert m["s_med"] <= 1e-5 and m["s_tail"] <= 1e-3, (cfg, m)
    assert m["c_med"] <= 4 * m["s_med"] and m["c_tail"] <= 4 * m["s_tail"], (cfg, m)


@pytest.mark.parametrize("cfg,abbe", CASES, ids=["C2", "C3-V50", "C5"])
def test_wavelength_tangent_ratio_to_its_own_size(cfg, abbe, driver, oracle_lib):
    """The check as the issue set it: |got - ref| / max(|ref|, 1e-3 of the batch's median |ref|) per 3-vector, median and 99.9th
    percentile at most 4 x the screen tangents' figures on the same rays.

    The tangent is traced in f64 because of this check.  A lens is achromatised by making the crown and flint contributions cancel, so
    the tangent is the small remainder of its source terms (last column); traced in f32 it carried their rounding times that factor and
    missed the bound by far (second column).  Measured (host build; median / 99.9th percentile):

                            screen tangents      wavelength tangent, f32 trace (ratio)    f64 trace (ratio)              sum |contributions| / |dD/dlambda|
        C2 Tessar           2.4e-7 / 5.6e-6      6.6e-6 / 2.9e-4  (27 / 52)               2.9e-8 / 9.3e-8 (0.12 / 0.02)  46
        C3 dbl Gauss V=50   3.0e-7 / 1.8e-6      7.4e-7 / 2.4e-5  (2.5 / 13)              2.6e-8 / 7.6e-8 (0.09 / 0.04)  4.6
        C5 Petzval          3.2e-7 / 1.6e-6      1.4e-6 / 1.3e-4  (4.3 / 83)              2.6e-8 / 8.8e-8 (0.08 / 0.06)  25

    What is left is the rounding of the six results to f32."""
    m = _measure(cfg, abbe, driver, oracle_lib)
    assert m["l_med"] <= 4 * m["s_med"] and m["l_tail"] <= 4 * m["s_tail"], (cfg, m)


@pytest.mark.parametrize("cfg,abbe", CASES, ids=["C2", "C3-V50", "C5"])
def test_d_line_gives_the_d_line_tangents(cfg, abbe, driver, oracle_lib):
    """at lambda = 587.5618f the screen tangents are kolb_differentials', bit for bit, on every ray"""
    p, info, disp, surf, hs = tables(cfg, abbe)
    o, d = _rays(cfg, oracle_lib)
    lam = np.full(len(o), LAMBDA_D32, F32)
    ref, _, rprim = run_driver(driver, 0, surf, disp, hs, lam, o, d)
    for mode in (1, 2):
        got, _, prim = run_driver(driver, mode, surf, disp, hs, lam, o, d)
        assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(prim), _bits(rprim))


def test_lens_without_v_numbers(driver, oracle_lib):
    """4-column prescription (every B = 0): any valid wavelength gives the d-line tangents bit for bit and a wavelength tangent of
    exactly +0.0 or -0.0"""
    p, info, disp, surf, hs = tables("C3")
    assert not disp["cauchy_b"].any()
    o, d = _rays("C3", oracle_lib)
    lam = np.random.RandomState(3).uniform(360, 830, len(o)).astype(F32)
    lam[:2] = [360.0, 830.0]
    ref, _, _ = run_driver(driver, 0, surf, disp, hs, lam, o, d)
    got, chroma, _ = run_driver(driver, 2, surf, disp, hs, lam, o, d)
    assert np.array_equal(_bits(got), _bits(ref))
    assert not (_bits(chroma) & np.uint32(0x7FFFFFFF)).any()


@pytest.mark.parametrize("lam_nm", [420.0, 680.0])
def test_the_d_line_tangents_miss_the_spectral_path(lam_nm, driver, oracle_lib):
    """Why the call exists, on the shipped TESSAR: against the f64 reference at 420 / 680 nm the d-line call's dDdx and dDdy miss by
    more than the spectral call's bound on a ray (1e-3; its median bound is 1e-5) on more than half of the rays, while the spectral call is
    within its bounds (median <= 1e-5, 99.9th percentile <= 1e-3)."""
    p, info, disp, surf, hs = tables("C2")
    o, d = _rays("C2", oracle_lib)
    lam = np.full(len(o), lam_nm, F32)
    ok = _passes(surf, sref.cauchy_eta(disp, lam), o, d)
    o, d, lam = o[ok], d[ok], lam[ok]
    fd = sref.jacobian_fd(surf, disp, lam, hs, o, d)
    dline, _, _ = run_driver(driver, 0, surf, disp, hs, lam, o, d)
    spec, _, _ = run_driver(driver, 1, surf, disp, hs, lam, o, d)
    miss = dref.rel_err(dline, fd)[:, 2:]
    e = dref.rel_err(spec, fd)[:, 2:]
    print("%g nm: d-line miss median %.2e, share > 1e-5 %.3f, share > 1e-3 %.3f; spectral %.2e / %.2e" %
          (lam_nm, float(np.median(miss)), float((miss > 1e-5).mean()), float((miss > 1e-3).mean()), float(np.median(e)),
           float(np.percentile(e, 99.9))))
    assert (miss > 1e-3).all(1).mean() > 0.5
    assert np.median(e) <= 1e-5 and np.percentile(e, 99.9) <= 1e-3


def _singlet():
    return tables("C2", lens_text=SINGLET, focalLength=5.0, fStop=4.0, kolbSamplingLUT=False, focalDistance=100.0)


def _marginal_rays(info, n=2000):
    """an on-axis sensor point aimed at the lens's outer zone (the lens point lies |thickness[0]| in front of the sensor point, the
    glass six times as far: the rays that get through aim within 0.09 of the rear aperture)"""
    el = info["elements"]
    rs = np.random.RandomState(9)
    r = rs.uniform(0.045, 0.085, n) * el[0, 3]
    a = rs.uniform(0, 2 * np.pi, n)
    o = np.tile(np.array([0.0, 0.0, info["originShift"]], F32), (n, 1))
    d = np.stack([r * np.cos(a), r * np.sin(a), np.full(n, -el[0, 1])], 1).astype(F32)
    return o, d


def test_wavelength_tangent_sign_blue_focuses_closer(driver):
    """test_blue_focuses_closer_than_red in derivative form: for marginal rays of the singlet (V = 30) from the on-axis sensor point, the
    ray parameter t = -(O.D)xy / |Dxy|^2 of the axis crossing in object space grows with the wavelength"""
    p, info, disp, surf, hs = _singlet()
    o, d = _marginal_rays(info)
    lam = np.full(len(o), LAMBDA_D32, F32)
    ok = _passes(surf, sref.cauchy_eta(disp, lam), o, d, info["elements"][:, 3])
    assert ok.mean() > 0.9
    o, d, lam = o[ok], d[ok], lam[ok]
    _, chroma, prim = run_driver(driver, 2, surf, disp, hs, lam, o, d)
    O, D, dO, dD = (a.astype(np.float64) for a in (prim[:, 0:3], prim[:, 3:6], chroma[:, 0:3], chroma[:, 3:6]))
    od = (O[:, :2] * D[:, :2]).sum(1)
    rho2 = (D[:, :2] ** 2).sum(1)
    dt = -((dO[:, :2] * D[:, :2]).sum(1) + (O[:, :2] * dD[:, :2]).sum(1)) / rho2 + od * 2 * (D[:, :2] * dD[:, :2]).sum(1) / rho2 ** 2
    assert (dt > 0).all(), float((dt > 0).mean())
    # and the same from the f64 reference's own rays at 450 / 650 nm
    t = {}
    for w in (450.0, 650.0):
        ro, rd, _ = sref.trace(surf, sref.cauchy_eta(disp, np.full(len(o), w)), o, d)
        t[w] = (ro[:, :2] * rd[:, :2]).sum(1) / -(rd[:, :2] ** 2).sum(1)
    assert (t[450.0] < t[650.0]).all()


def _quadrature_weights(a, m, b):
    """weights of the integral over [a, b] of the parabola through values at a, m, b (Simpson's rule where m is the midpoint)"""
    V = np.array([[1.0, 1.0, 1.0], [a, m, b], [a * a, m * m, b * b]])
    return np.linalg.solve(V, np.array([b - a, (b * b - a * a) / 2, (b ** 3 - a ** 3) / 3]))


def test_wavelength_tangent_integrates_to_the_colour_shift(driver):
    """D(C) - D(F) of the singlet's marginal rays against the integral of dD/dlambda over [F, C] by the three-point rule on the tangent
    at F, d and C (Simpson's rule for nodes that are not equally spaced: the d-line is not the midpoint).  The rule itself errs because
    the Cauchy index is not a parabola in lambda: with the f64 reference's own tangent (its central difference) at the three nodes it
    misses the f64 D(C) - D(F) by 5.06e-3 of its length (median over the rays; 5.05e-3 ... 5.07e-3 from the best ray to the worst).  The
    host build's tangents must give the reference's integral within 1e-4 of the shift (measured 5.8e-8) and so meet the f64 shift within the rule's own error plus that."""
    p, info, disp, surf, hs = _singlet()
    o, d = _marginal_rays(info)
    nodes = (sref.LAMBDA_F, sref.LAMBDA_D, sref.LAMBDA_C)
    ok = np.ones(len(o), bool)
    for w in nodes:
        ok &= _passes(surf, sref.cauchy_eta(disp, np.full(len(o), w)), o, d, info["elements"][:, 3])
    assert ok.mean() > 0.9
    o, d = o[ok], d[ok]
    wq = _quadrature_weights(*nodes)
    end = {}
    got = np.zeros((len(o), 3))
    ref = np.zeros((len(o), 3))
    for w, q in zip(nodes, wq):
        lam = np.full(len(o), w, F32)
        _, chroma, _ = run_driver(driver, 2, surf, disp, hs, lam, o, d)
        got += q * chroma[:, 3:6].astype(np.float64)
        ref += q * sref.wavelength_fd(surf, disp, lam, o, d)[:, 3:6]
        end[w] = -sref.trace(surf, sref.cauchy_eta(disp, lam), o, d)[1]
    shift = end[sref.LAMBDA_C] - end[sref.LAMBDA_F]
    size = np.linalg.norm(shift, axis=1)
    rule = np.linalg.norm(ref - shift, axis=1) / size
    lib = np.linalg.norm(got - shift, axis=1) / size
    same = np.linalg.norm(got - ref, axis=1) / size
    print("rule's own error %.3e (%.3e ... %.3e), host build %.3e, host build against the reference's integral %.2e" %
          (float(np.median(rule)), float(rule.min()), float(rule.max()), float(np.median(lib)), float(same.max())))
    assert size.min() > 1e-4                       # there is a colour shift to integrate
    assert same.max() <= 1e-4
    assert 4e-3 < np.median(rule) < 6e-3           # the figure stated above
    assert np.median(lib) <= np.median(rule) + 1e-4


def test_spectral_differential_kernels_budget():
    """0 scratch and 0 VGPR spills for every spectral differential kernel of the built library (its code object's metadata), at most
    128 VGPRs for the 12-float ones; the d-line pass still has its four kernels"""
    all_k = kernel_resources()
    res = {k: v for k, v in all_k.items() if "spectral_diff" in k}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        if "<false>" in k:
            assert v["vgpr"] + v["agpr"] <= 128, (k, v)
    assert sum("<false>" in k for k in res) == 2
    assert len([k for k in all_k if "differentials_kernel" in k]) == 4

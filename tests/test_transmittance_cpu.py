"""Fresnel transmittance of traced rays without a GPU: the C-ABI declares and exports the three calls and answers a tables-only camera
as the header says, the arithmetic of csrc/transmittance.hpp (compiled for the host) agrees with the f64 numpy restatement
(transmittance_ref.py) from the same starts, the film's cosine polynomial holds against f64, the physics is what a lens designer
expects (the on-axis closed form, Brewster's angle, the ideal quarter-wave film), and the gfx950 kernels keep their budget.

Rays: differentials_spectral_ref.lens_rays (~10 k passing rays per lens, C2 - C5) with ray_wavelengths; no ray is left out.  The measured
figures are in test_host_build_against_f64."""
import ctypes
import os
import re

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import LENS_DIR, ZoicCamera, ZoicError

import host_drivers
import transmittance_ref as tref
from device_cases import bits_f32 as _bits
from differentials_spectral_ref import lens_rays as _rays, ray_wavelengths as _wavelengths, tables
from host_drivers import run_transmittance as run_driver
from library_facts import header_text, kernel_resources
from transmittance_ref import FILM_INDEX, FILM_LAMBDA0, LENSES, films_where_media_differ, housings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zoic_ray_transmittance_device", "zoic_camera_set_coatings", "zoic_camera_get_coatings")
F32 = np.float32
LAMBDA_D32 = F32(587.5618)
INVALID = _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
NO_DEVICE = _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")

# Largest |host build - f64 restatement| of T over the eight runs of test_host_build_against_f64 (clang++ 22, x86-64) and the bound
# asserted there and wherever "the bound" is said below: 4 x it, the margin for other compilers' host builds
MEASURED = 3.354e-7
BOUND = 4 * MEASURED
# Largest |film_cospi - cos(pi x)| on 10^5 points of [0, 2.31] and what is asserted: the polynomial is exact arithmetic of the same
# operations everywhere (fmaf, one rounding each), so the margin only covers other points than these
COSPI_MEASURED = 1.014e-7
COSPI_BOUND = 2e-7


def test_abi_declares_and_exports_the_calls():
    text = header_text()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS and hasattr(raw, name) and hasattr(_capi.load(), name), name
    assert len(_capi.SYMBOLS[NAMES[0]][1]) == 10 and len(_capi.SYMBOLS[NAMES[1]][1]) == 4 and len(_capi.SYMBOLS[NAMES[2]][1]) == 4
    assert "zoic_ray_transmittance_device" in open(os.path.join(ROOT, "include", "zoic_amd.h")).read().split("#define ZOIC_AMD_ABI_VERSION")[0]
    assert _capi.load().zoic_abi_version() == 5 and _capi.ABI_VERSION == 5


@pytest.fixture(scope="module")
def driver():
    return host_drivers.transmittance()


# ---- the interface on a tables-only camera --------------------------------------------------------------------------------------
def test_errors_on_a_tables_only_camera():
    lib = _capi.load()
    p, info, disp, surf, hs = tables("C2")
    cam = ZoicCamera(device=-1)
    cam.update(**p)
    count = info["lensCount"]
    f = lib.zoic_ray_transmittance_device
    for k in (0, 9):      # checked first, on every camera
        assert f(cam._h, 64, k, None, None, None, 0, None, None, None) == INVALID
        assert f(cam._h, 0, k, None, None, None, 0, None, None, None) == INVALID
    assert f(None, 64, 1, None, None, None, 0, None, None, None) == INVALID
    assert f(cam._h, 64, 1, None, None, None, 0, None, None, None) == NO_DEVICE
    nc, l0 = np.full(count, 1.38, F32), np.full(count, 550.0, F32)
    P = lambda a: a.ctypes.data
    s = lib.zoic_camera_set_coatings
    assert s(None, count, P(nc), P(l0)) == INVALID
    assert s(cam._h, count, None, P(l0)) == INVALID and s(cam._h, count, P(nc), None) == INVALID
    assert s(cam._h, count + 1, P(np.resize(nc, count + 1)), P(np.resize(l0, count + 1))) == INVALID
    assert s(cam._h, -1, P(nc), P(l0)) == INVALID and s(cam._h, 33, P(np.resize(nc, 33)), P(np.resize(l0, 33))) == INVALID
    for bad_nc, bad_l0 in ((0.5, 550.0), (np.nan, 550.0), (np.inf, 550.0), (-1.38, 550.0), (1.38, 0.0), (1.38, -550.0), (1.38, np.nan),
                           (1.38, np.inf)):
        a, b = nc.copy(), l0.copy()
        a[3], b[3] = bad_nc, bad_l0
        assert s(cam._h, count, P(a), P(b)) == INVALID, (bad_nc, bad_l0)
    assert not cam.coatings()["index"].any()                 # nothing was taken from the refused calls
    a, b = nc.copy(), l0.copy()
    a[2], b[2] = 0.0, np.nan                                 # uncoated: its lambda0 is not looked at
    assert s(cam._h, count, P(a), P(b)) == 0
    assert lib.zoic_camera_get_coatings(None, 0, None, None) == -1 and lib.zoic_camera_get_coatings(cam._h, -1, None, None) == -1
    assert s(cam._h, 0, None, None) == 0 and not cam.coatings()["index"].any()
    cam.close()


def test_coatings_order_default_and_update():
    """get_coatings: trace order = reversed file order; the default is all uncoated; the override survives an update of the same lens and
    fails one whose lens has another surface count, like zoic_camera_set_abbe_numbers'"""
    p, info, disp, surf, hs = tables("C2")
    count = info["lensCount"]
    cam = ZoicCamera(device=-1)
    assert cam.coatings()["index"].shape == (0,)              # no lens yet
    nc = (1.3 + 0.01 * np.arange(count)).astype(F32)
    l0 = (500.0 + np.arange(count)).astype(F32)
    nc[1] = 0.0
    cam.set_coatings(nc, l0)                                   # before the first update: any count is taken
    cam.update(**p)
    got = cam.coatings()
    assert np.array_equal(got["index"], nc[::-1]) and np.array_equal(got["lambda0_nm"][nc[::-1] != 0], l0[::-1][nc[::-1] != 0])
    assert got["lambda0_nm"][count - 2] == 0.0
    cam.update(**dict(p, fStop=8.0))
    assert np.array_equal(cam.coatings()["index"], nc[::-1])
    p3 = tables("C3")[0]
    assert tables("C3")[1]["lensCount"] != count
    with pytest.raises(ZoicError) as e:
        cam.update(**p3)
    assert e.value.status == INVALID and "zoic_camera_set_coatings" in str(e.value)
    cam.set_coatings(None, None)
    cam.update(**p3)
    assert not cam.coatings()["index"].any() and len(cam.coatings()["index"]) == tables("C3")[1]["lensCount"]
    with pytest.raises(ZoicError):
        cam.set_coatings(nc, l0)                               # a loaded lens: the count must be its own
    cam.set_coatings(np.full(len(cam.coatings()["index"]), 1.38, F32), 550.0)     # a scalar lambda0 serves all
    assert (cam.coatings()["lambda0_nm"] == 550.0).all()
    cam.close()
    wrong = ZoicCamera(device=-1)
    wrong.set_coatings(nc[:3], l0[:3])
    with pytest.raises(ZoicError):
        wrong.update(**p)
    wrong.close()


# ---- against f64 ----------------------------------------------------------------------------------------------------------------
CFGS = ["C2", "C3", "C4", "C5"]
_MEASURED = {}


def _measure(cfg, coated, driver, oracle_lib):
    key = (cfg, coated)
    if key not in _MEASURED:
        p, info, disp, surf, hs = tables(cfg)
        o, d = _rays(cfg, oracle_lib)
        lam = _wavelengths(len(o))
        film = films_where_media_differ(disp) if coated else None
        ref, ok = tref.transmittance(surf, disp, lam, o, d, *(film or (None, None)))
        assert ok.all(), (cfg, int((~ok).sum()))                          # no ray is left out
        got = run_driver(driver, surf, disp, lam, o, d, film)
        assert (got > 0).all() and (got < 1).all()
        err = np.abs(got.astype(np.float64) - ref)
        _MEASURED[key] = dict(n=len(o), err=float(err.max()), t_min=float(ref.min()), t_med=float(np.median(ref)))
        print(cfg, "coated" if coated else "bare", _MEASURED[key])
    return _MEASURED[key]


@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("cfg", CFGS)
def test_host_build_against_f64(cfg, coated, driver, oracle_lib):
    """|host build - f64 restatement| of T from the same starts, every ray, at most BOUND = 4 x the largest error measured over these
    eight runs.  Measured (largest absolute error; f64 T min / median):

                 bare                              1.38 / 550 nm film where the media differ
        C2       1.87e-7   0.665 / 0.685           2.41e-7   0.783 / 0.930
        C3       2.27e-7   0.579 / 0.588           2.80e-7   0.736 / 0.883
        C4       2.27e-7   0.517 / 0.532           3.35e-7   0.683 / 0.889
        C5       2.18e-7   0.634 / 0.657           2.83e-7   0.744 / 0.885

    The largest, 3.354e-7 (C4 with the film), is MEASURED; BOUND = 1.34e-6.  Film cosine: 1.014e-7 at x = 1.5016 (test_film_cosine)."""
    m = _measure(cfg, coated, driver, oracle_lib)
    assert m["err"] <= BOUND, m
    # the figures this feature was asked for with: a third to a half of the light is lost bare, about a tenth with the film
    if not coated:
        assert 0.5 < m["t_min"] <= m["t_med"] < 0.7, m
    else:
        assert 0.86 < m["t_med"] < 0.94, m


def test_measured_bound_is_the_measured_one(driver, oracle_lib):
    """MEASURED is what these eight runs give on the build it was taken from, not a round figure: the largest error lies within
    [MEASURED / 4, 4 MEASURED] on any host build"""
    worst = max(_measure(cfg, coated, driver, oracle_lib)["err"] for cfg in CFGS for coated in (False, True))
    assert MEASURED / 4 <= worst <= BOUND, worst


def test_film_cosine(driver):
    x = np.linspace(0.0, 2.31, 100000).astype(F32)
    y = np.zeros_like(x)
    fp = ctypes.POINTER(ctypes.c_float)
    driver.ztr_cospi(len(x), x.ctypes.data_as(fp), y.ctypes.data_as(fp))
    err = np.abs(y.astype(np.float64) - np.cos(np.pi * x.astype(np.float64)))
    print("film cosine: largest error %.3e at x = %.6f" % (float(err.max()), float(x[err.argmax()])))
    assert err.max() <= COSPI_BOUND
    # beyond the film's range the reduction still holds (a lambda0 in the infrared)
    x = np.linspace(2.31, 40.0, 100000).astype(F32)
    driver.ztr_cospi(len(x), x.ctypes.data_as(fp), y.ctypes.data_as(fp))
    assert np.abs(y.astype(np.float64) - np.cos(np.pi * x.astype(np.float64))).max() <= COSPI_BOUND
    one = np.array([0.0, 1.0, 2.0, 0.5, 1.5], F32)
    out = np.zeros_like(one)
    driver.ztr_cospi(5, one.ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert np.array_equal(out, np.array([1.0, -1.0, 1.0, 0.0, 0.0], F32)) or np.abs(out - [1, -1, 1, 0, 0]).max() <= COSPI_BOUND


# ---- physics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", LENSES)
def test_on_axis_ray_is_the_closed_form(lens, driver):
    """a ray along the axis of every shipped prescription, bare, at lambda_d: prod 1 - ((n1 - n2) / (n1 + n2))^2 on the camera's own
    ior_d, to the bound"""
    p, info, disp, surf, hs = tables("C2", lensDataPath=os.path.join(LENS_DIR, lens))
    o = np.array([[0.0, 0.0, info["originShift"]]], F32)
    d = np.array([[0.0, 0.0, -info["elements"][0, 1]]], F32)
    got = run_driver(driver, surf, disp, np.array([LAMBDA_D32]), o, d, housing2=housings(info))
    want = tref.on_axis_closed_form(disp["ior_d"])
    print(lens, float(got[0]), want)
    assert abs(float(got[0]) - want) <= BOUND
    assert 0.3 < want < 0.95


def test_on_axis_figures_of_three_prescriptions():
    """the closed form on three shipped prescriptions, as DESIGN 4.15 quotes it"""
    for lens, want in (("tessar_f2.8.dat", 0.6872), ("double_gauss_f2.0.dat", 0.5900), ("petzval_f1.25.dat", 0.6597)):
        disp = tables("C2", lensDataPath=os.path.join(LENS_DIR, lens))[2]
        assert abs(tref.on_axis_closed_form(disp["ior_d"]) - want) < 5e-5, lens


def _flat(n_glass, film=(0.0, 0.0), b=0.0):
    """one nearly flat interface (|R| = 1e4, like the stop's sphere) at z = 0 between glass (behind: the ray comes from there) and air"""
    R = F32(1e4)
    surf = np.array([[R, R * R, 1.0, 1.0]], F32)
    disp = dict(ior_d=np.array([n_glass], F32), cauchy_b=np.array([b], F32))
    return surf, disp, (np.array([film[0]], F32), np.array([film[1]], F32))


def test_brewster_angle(driver):
    """at Brewster's angle (tan i = n2 / n1) the reflected light is all s-polarised: R_p below the bound, so T = 1 - R_s / 2 -- through
    the interface function on the exact angle's cosines, and through the trace at one flat-enough interface from glass into air"""
    n1, n2 = 1.5, 1.0
    i = np.arctan(n2 / n1)
    ci, ct = np.cos(i), np.sin(i)                          # cos t = sin i there
    rs2 = ((n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)) ** 2
    t = driver.ztr_interface(n1, n2, ci, ct, 0.0, 0.0, 550.0)
    assert abs(2 * (1 - t) - rs2) <= 2 * BOUND             # R_s + R_p - R_s = R_p
    surf, disp, film = _flat(n1)
    o = np.array([[0.0, 0.0, 1.0]], F32)
    d = np.array([[np.sin(i), 0.0, -np.cos(i)]], F32)
    got = run_driver(driver, surf, disp, np.array([LAMBDA_D32]), o, d)
    ref, ok = tref.transmittance(surf, disp, [LAMBDA_D32], o, d)
    assert ok.all() and abs(float(got[0]) - float(ref[0])) <= BOUND
    assert abs(2 * (1 - float(got[0])) - rs2) <= 1e-4     # the sphere's normal is 1e-4 off the axis at this hit


def test_ideal_quarter_wave_film(driver):
    """nc = sqrt(n1 n2) at normal incidence and lambda = lambda0: no reflection; away from lambda0 some, but less than bare"""
    n1, n2 = 1.0, 1.5
    nc = float(np.sqrt(n1 * n2))
    assert abs(driver.ztr_interface(n1, n2, 1.0, 1.0, nc, 550.0, 550.0) - 1.0) <= BOUND
    bare = driver.ztr_interface(n1, n2, 1.0, 1.0, 0.0, 0.0, 550.0)
    assert abs(bare - 0.96) <= BOUND
    off = driver.ztr_interface(n1, n2, 1.0, 1.0, nc, 550.0, 400.0)
    assert bare < off < 1.0
    # a half-wave film (lambda = lambda0 / 2) is absent at normal incidence
    assert abs(driver.ztr_interface(n1, n2, 1.0, 1.0, 1.38, 800.0, 400.0) - bare) <= BOUND
    # evanescent in the film: the bare interface's value, bit for bit
    ci = float(np.cos(np.radians(70.0)))
    ct = float(np.sqrt(1 - (1.7 / 1.6) ** 2 * (1 - ci * ci)))
    assert (1.7 / 1.05) ** 2 * (1 - ci * ci) > 1
    assert driver.ztr_interface(1.7, 1.6, ci, ct, 1.05, 550.0, 500.0) == driver.ztr_interface(1.7, 1.6, ci, ct, 0.0, 0.0, 500.0)


def test_film_between_equal_media_changes_no_bit(driver, oracle_lib):
    """a film on the stop (air on both sides) is ignored: coated where the media differ == coated everywhere, bit for bit; and the
    film does change the bits where it counts"""
    p, info, disp, surf, hs = tables("C2")
    o, d = _rays("C2", oracle_lib)
    lam = _wavelengths(len(o))
    some = films_where_media_differ(disp)
    assert (some[0] == 0).any()                              # the stop
    every = (np.full(len(surf), FILM_INDEX, F32), np.full(len(surf), FILM_LAMBDA0, F32))
    a, b = run_driver(driver, surf, disp, lam, o, d, some), run_driver(driver, surf, disp, lam, o, d, every)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(a), _bits(run_driver(driver, surf, disp, lam, o, d)))


def test_no_path_gives_plus_zero(driver):
    """totally reflected, clipped, past the sphere: exactly +0.0; the same starts with room to pass: T > 0"""
    surf, disp, film = _flat(1.5)
    lam = np.array([LAMBDA_D32])
    steep = np.array([[np.sin(np.radians(60.0)), 0.0, -np.cos(np.radians(60.0))]], F32)     # beyond the critical angle (41.8 deg)
    gentle = np.array([[0.2, 0.0, -1.0]], F32)
    o = np.array([[0.0, 0.0, 1.0]], F32)
    t = run_driver(driver, surf, disp, lam, o, steep)
    assert _bits(t)[0] == 0
    assert run_driver(driver, surf, disp, lam, o, gentle)[0] > 0.9
    t = run_driver(driver, surf, disp, lam, o, gentle, housing2=[0.01])                     # hits at x = 0.2: h2 = 0.04
    assert _bits(t)[0] == 0
    assert run_driver(driver, surf, disp, lam, o, gentle, housing2=[0.05])[0] > 0.9
    small = np.array([[0.0, 1.0, 1.0, np.inf]], F32)                                        # a unit sphere about the origin
    t = run_driver(driver, small[:, :4], disp, lam, np.array([[3.0, 0.0, 5.0]], F32), np.array([[0.0, 0.0, -1.0]], F32))
    assert _bits(t)[0] == 0
    # the real lens: a start aimed past the rear element is clipped there
    p, info, disp2, surf2, hs = tables("C2")
    el = info["elements"]
    o2 = np.array([[0.0, 0.0, info["originShift"]]], F32)
    d2 = np.array([[el[0, 3] * 2.0, 0.0, -el[0, 1]]], F32)
    assert _bits(run_driver(driver, surf2, disp2, lam, o2, d2, housing2=housings(info)))[0] == 0


def test_d_line_is_any_wavelength_on_a_lens_without_v_numbers(driver, oracle_lib):
    """C3 ships no V-numbers (every B = 0): bare, every valid wavelength gives the d-line's T bit for bit; the film still sees it"""
    p, info, disp, surf, hs = tables("C3")
    assert not disp["cauchy_b"].any()
    o, d = _rays("C3", oracle_lib)
    lam = _wavelengths(len(o))
    dline = np.full(len(o), LAMBDA_D32, F32)
    assert np.array_equal(_bits(run_driver(driver, surf, disp, lam, o, d)), _bits(run_driver(driver, surf, disp, dline, o, d)))
    film = films_where_media_differ(disp)
    assert not np.array_equal(_bits(run_driver(driver, surf, disp, lam, o, d, film)), _bits(run_driver(driver, surf, disp, dline, o, d, film)))


def test_transmittance_kernels_budget():
    """0 scratch, 0 VGPR spills and at most 128 VGPRs for the transmittance kernels of the built library (its code object's metadata);
    the kernel arguments fit their 4 KB"""
    res = {k: v for k, v in kernel_resources().items() if "transmittance" in k}
    assert len(res) == 2, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert v["vgpr"] + v["agpr"] <= 128, (k, v)
        assert v["kernarg"] <= 4096, (k, v)

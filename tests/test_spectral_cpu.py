"""Rays at a wavelength per ray without a GPU: the C-ABI declares and exports the spectral calls, the dispersion table of every shipped
lens equals a numpy restatement bit for bit (V-number override and its checks included), the per-ray index / eta / TIR arithmetic of
csrc/spectral.hpp (compiled for the host) equals its numpy restatement bitwise, and the new gfx950 kernels neither spill nor use
scratch."""
import ctypes
import os
import re

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera, ZoicError, lens_path
from zoic_amd.workloads import camera_params

import host_drivers
from library_facts import header_text, kernel_resources
from spectral_ref import LAMBDA_C, LAMBDA_D, LAMBDA_F, cauchy_b, interface_terms, spectral_iors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zoic_create_rays_spectral_device", "zoic_camera_get_dispersion", "zoic_camera_set_abbe_numbers")
LENSES = sorted(f for f in os.listdir(os.path.join(ROOT, "zoic_amd", "lenses")) if f.endswith(".dat"))
# the prescriptions a camera can load: zoic rejects a lens without an aperture row (radius 0, zoic.cpp:922)
LOADABLE = [f for f in LENSES if any(l.split() and float(l.split()[0]) == 0.0 for l in open(os.path.join(ROOT, "zoic_amd", "lenses", f))
                                     if not l.lstrip().startswith("#"))]


def test_abi_declares_and_exports_spectral_calls():
    text = header_text()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert _capi.load().zoic_abi_version() == 5


def _file_abbe(path):
    """the prescription's V column in trace order (rear first); zeros for a 4-column file"""
    rows = [l.split() for l in open(path) if l.strip() and not l.lstrip().startswith("#")]
    v = [float(r[3]) if len(r) == 5 else 0.0 for r in rows]
    return np.array(v[::-1], np.float32)


def _camera(lens, **over):
    p = dict(camera_params("C2"), lensDataPath=lens_path(lens))
    p.update(over)
    cam = ZoicCamera(device=-1)
    cam.update(**p)
    return cam, p


@pytest.mark.parametrize("lens", LOADABLE)
def test_dispersion_table_matches_numpy(lens):
    cam, _ = _camera(lens)
    d = cam.dispersion()
    info = cam.info()
    n = info["lensCount"]
    assert len(d["ior_d"]) == n
    assert np.array_equal(d["ior_d"], info["elements"][:, 2])
    abbe = _file_abbe(lens_path(lens))
    assert np.array_equal(d["abbe"], abbe)
    want = cauchy_b(d["ior_d"], abbe)
    assert np.array_equal(d["cauchy_b"].view(np.uint32), want.view(np.uint32))
    assert not d["cauchy_b"][d["ior_d"] == 1.0].any()                 # air: no dispersion
    if not abbe.any():
        assert not d["cauchy_b"].any()                                 # 4-column prescription
    glass = d["cauchy_b"] != 0
    # the Abbe number's definition: n(F) - n(C) = (n_d - 1) / V -- of the model (B in f64) to 1e-6, of the per-ray f32 indices to
    # their rounding (a few ulps of n ~ 1.6)
    want = (d["ior_d"][glass].astype(np.float64) - 1.0) / abbe[glass]
    model = d["cauchy_b"][glass].astype(np.float64) * (1.0 / LAMBDA_F ** 2 - 1.0 / LAMBDA_C ** 2)
    assert np.all(np.abs(model - want) <= 1e-6 * want)
    nF = spectral_iors(d["ior_d"], d["cauchy_b"], LAMBDA_F).astype(np.float64)
    nC = spectral_iors(d["ior_d"], d["cauchy_b"], LAMBDA_C).astype(np.float64)
    assert np.all(np.abs((nF - nC)[glass] - want) <= 4.0 * 2.0 ** -23 * 2.0)
    cam.close()


def test_four_column_lenses_ship():
    four = [l for l in LOADABLE if not _file_abbe(lens_path(l)).any()]
    assert "double_gauss_f2.0.dat" in four and "fisheye_muller_f4.0.dat" in four


def test_abbe_override_in_file_order():
    cam, p = _camera("double_gauss_f2.0.dat")
    n = cam.info()["lensCount"]
    V = np.linspace(30.0, 70.0, n).astype(np.float32)     # front to rear
    cam.set_abbe_numbers(V)
    d = cam.dispersion()
    assert np.array_equal(d["abbe"], V[::-1])             # trace order: rear first
    assert np.array_equal(d["cauchy_b"].view(np.uint32), cauchy_b(d["ior_d"], V[::-1]).view(np.uint32))
    assert d["cauchy_b"].any() and not d["cauchy_b"][d["ior_d"] == 1.0].any()
    cam.update(**p)                                       # the override survives an update of the same lens
    assert np.array_equal(cam.dispersion()["abbe"], V[::-1])
    cam.set_abbe_numbers(None)
    assert not cam.dispersion()["cauchy_b"].any()
    cam.close()


def test_abbe_override_count_is_checked():
    cam, p = _camera("tessar_f2.8.dat")
    n = cam.info()["lensCount"]
    with pytest.raises(ZoicError) as e:
        cam.set_abbe_numbers(np.full(n + 1, 50.0, np.float32))
    assert e.value.status_name == "ZOIC_ERR_INVALID_ARGUMENT"
    cam.set_abbe_numbers(np.full(n, 50.0, np.float32))
    # checked again at every update: a lens of another surface count
    other = dict(p, lensDataPath=lens_path("double_gauss_f2.0.dat"))
    assert ZoicCamera(device=-1).update(**other).info()["lensCount"] != n
    with pytest.raises(ZoicError) as e:
        cam.update(**other)
    assert e.value.status_name == "ZOIC_ERR_INVALID_ARGUMENT"
    cam.set_abbe_numbers(None)
    cam.update(**other)
    cam.close()
    # before any lens: accepted, then checked by the update
    fresh = ZoicCamera(device=-1)
    fresh.set_abbe_numbers([50.0, 40.0])
    with pytest.raises(ZoicError):
        fresh.update(**p)
    fresh.close()


def test_abbe_override_changes_no_existing_table():
    cam, p = _camera("double_gauss_f2.0.dat")
    before = cam.info()
    cam.set_abbe_numbers(np.full(before["lensCount"], 40.0, np.float32))
    cam.update(**p)
    after = cam.info()
    for k in ("elements", "lutKeys", "lutBoxes", "originShift", "tracedFocalLength"):
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    cam.close()


@pytest.fixture(scope="module")
def driver():
    return host_drivers.spectral()


@pytest.mark.parametrize("lens,override", [("tessar_f2.8.dat", None), ("petzval_f1.25.dat", None), ("double_gauss_f2.0.dat", 50.0)])
def test_host_arithmetic_matches_numpy(driver, lens, override):
    cam, _ = _camera(lens)
    if override is not None:
        cam.set_abbe_numbers(np.full(cam.info()["lensCount"], override, np.float32))
    d = cam.dispersion()
    cam.close()
    count = len(d["ior_d"])
    lam = np.concatenate([np.linspace(360.0, 830.0, 2001, dtype=np.float32),
                          np.array([LAMBDA_D, LAMBDA_F, LAMBDA_C, np.nextafter(np.float32(360), 0), np.nan, np.inf, 0.0, -500.0,
                                    np.nextafter(np.float32(830), np.float32(1e4))], np.float32)])
    n = len(lam)
    out = {k: np.zeros((n, count), np.float32) for k in ("ior1", "ior2", "eta")}
    tir = np.zeros((n, count), np.int32)
    valid = np.zeros(n, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    driver.zs_terms(count, P(d["ior_d"]), P(d["cauchy_b"]), n, P(lam), P(out["ior1"]), P(out["ior2"]), P(out["eta"]), P(tir), P(valid))
    for r in range(n):
        if not (lam[r] >= 360.0 and lam[r] <= 830.0):
            assert valid[r] == 0, lam[r]
            continue
        assert valid[r] == 1, lam[r]
        i1, i2, eta, t = interface_terms(d["ior_d"], d["cauchy_b"], lam[r])
        assert np.array_equal(out["ior1"][r].view(np.uint32), i1.view(np.uint32)), lam[r]
        assert np.array_equal(out["ior2"][r].view(np.uint32), i2.view(np.uint32)), lam[r]
        assert np.array_equal(out["eta"][r].view(np.uint32), eta.view(np.uint32)), lam[r]
        assert np.array_equal(tir[r] != 0, t), lam[r]
    at_d = np.nonzero(lam == LAMBDA_D)[0][0]
    assert np.array_equal(out["ior1"][at_d].view(np.uint32), d["ior_d"].view(np.uint32))   # the d-line is n_d exactly
    air = d["ior_d"] == 1.0
    assert (out["ior1"][valid == 1][:, air] == 1.0).all()                                  # air stays 1.0 everywhere
    if d["cauchy_b"].any():   # blue bends more: n rises towards short wavelengths
        g = np.argmax(d["cauchy_b"])
        assert out["ior1"][0, g] > out["ior1"][at_d, g] > out["ior1"][2000, g]


def test_spectral_kernels_budget():
    res = {k: v for k, v in kernel_resources().items() if "spectral" in k or "hero" in k}
    # one ray-kernel body, <FAST, HERO>: no instantiation may take more VGPRs than the separate spectral and hero kernels took before
    # they were merged
    caps = {"kolb_spectral_kernel<false, false>": 136, "kolb_spectral_kernel<true, false>": 138,
            "kolb_spectral_kernel<false, true>": 160, "kolb_spectral_kernel<true, true>": 161}
    for name, cap in caps.items():
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, (name, sorted(res))
        assert hits[0]["vgpr"] + hits[0]["agpr"] <= cap, (name, hits[0])
    assert any("spectral_reject_kernel" in k for k in res) and any("hero_replicate_kernel" in k for k in res), sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr_spill"] == 0, (k, v)

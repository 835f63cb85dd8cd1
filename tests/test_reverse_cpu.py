"""Reverse projection without a GPU: the C-ABI declares and exports the three calls, the new gfx950 kernel neither spills nor uses
scratch, the host build of csrc/reverse.hpp (compiled here with clang++) recovers the screen sample of points placed on f64 chief rays
of every shipped lens and of the thin lens, equals the library's zoic_project_point bit for bit, and handles the edge cases as the
header documents them.  zoic_camera_reverse_ray stays the reference's `return false` until a caller opts in."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera, ZoicError, lens_path
from zoic_amd.workloads import camera_params

import host_drivers
from host_drivers import drive_reverse as _drive
from library_facts import header_text, kernel_resources
from reverse_ref import BEHIND, MODEL_NONE, NON_FINITE, OUTSIDE, Lens, kolb_point_set, thin_point_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zoic_project_points_device", "zoic_project_point", "zoic_camera_set_reverse_projection")
LENSES = sorted(f for f in os.listdir(os.path.join(ROOT, "zoic_amd", "lenses")) if f.endswith(".dat"))
# the prescriptions a camera can load: zoic rejects a lens without an aperture row (radius 0, zoic.cpp:922)
LOADABLE = [f for f in LENSES if any(l.split() and float(l.split()[0]) == 0.0 for l in open(os.path.join(ROOT, "zoic_amd", "lenses", f))
                                     if not l.lstrip().startswith("#"))]


def _camera(lens=None, **over):
    p = camera_params("C1" if lens is None else "C2")
    if lens is not None:
        p["lensDataPath"] = lens_path(lens)
    p.update(over)
    cam = ZoicCamera(device=-1)
    cam.update(**p)
    return cam, p


def test_abi_declares_and_exports_reverse_calls():
    text = header_text()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert _capi.load().zoic_abi_version() == 5


def test_reverse_kernel_budget():
    res = {k: v for k, v in kernel_resources().items() if "project_points_kernel" in k}
    assert res, "project_points_kernel not in the library"
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr_spill"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)


@pytest.fixture(scope="module")
def driver():
    return host_drivers.reverse()


CASES = [(lens, fd) for lens in LOADABLE for fd in (100.0, 30.0)] + [(None, 100.0), (None, 30.0)]


@pytest.mark.parametrize("lens,fd", CASES)
def test_host_build_recovers_chief_ray_samples(driver, lens, fd):
    cam, p = _camera(lens, focalDistance=fd)
    if lens is None:
        pts, s, depth = thin_point_set(float(cam.info()["tan_fov"]), fd)
    else:
        pts, s, depth = kolb_point_set(cam.info(), p["sensorWidth"], fd)
    assert len(pts) >= 24 and (depth == 0).sum() >= 8   # (the Mori lens: a 12-sample image circle of unclipped chief rays)
    scr, fl = _drive(driver, cam, p, pts)
    # the library's host call is the same code: the same bits
    lib = np.array([cam.project_point(q) for q in pts[:: max(1, len(pts) // 512)]])
    assert np.array_equal(lib[:, :2].astype(np.float32).view(np.uint32), scr[:: max(1, len(pts) // 512)].view(np.uint32))
    assert np.array_equal(lib[:, 2].astype(np.uint32), fl[:: max(1, len(pts) // 512)])
    cam.close()
    proj = (fl & 1) == 1
    cover = proj.mean()
    if lens is not None and "fisheye" in lens:
        assert cover >= 0.999, cover
    else:
        assert cover == 1.0, (cover, np.unique(fl[~proj] >> 8, return_counts=True))
    err = np.abs(scr[proj].astype(np.float64) - s[proj]).max(1)
    # measured (every lens, both focus distances): max 9.6e-7, p99 6.6e-7 (fisheye); one pixel of a 3840-wide frame is 5.2e-4
    assert err.max() <= 1e-5, err.max()
    assert np.percentile(err, 99) <= 2e-6, np.percentile(err, 99)
    assert not (fl[proj] & 2).any()   # the set's chief rays are unclipped: so is what the projection traced


@pytest.mark.parametrize("lens", [None, "tessar_f2.8.dat", "fisheye_muller_f4.0.dat"])
def test_axis_projects_to_exact_zero(driver, lens):
    cam, p = _camera(lens)
    pts = np.array([[0.0, 0.0, -z] for z in (1.0, 100.0, 1e4, 1e30)] + [[-0.0, -0.0, -5.0]], np.float32)
    scr, fl = _drive(driver, cam, p, pts)
    assert (fl == 1).all(), fl
    assert (scr.view(np.uint32) == 0).all(), scr   # +0.0 exactly
    for q in pts:
        sx, sy, f = cam.project_point(q)
        assert f == 1 and np.float32(sx).view(np.uint32) == 0 and np.float32(sy).view(np.uint32) == 0
    cam.close()


def _reason(f):
    return (int(f) >> 8) & 15


@pytest.mark.parametrize("lens", [None, "double_gauss_f2.0.dat"])
def test_edge_cases_are_not_projected(driver, lens):
    cam, p = _camera(lens)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cases = [((0.1, 0.2, 1.0), BEHIND), ((0.1, 0.2, 0.0), BEHIND), ((nan, 0.0, -10.0), NON_FINITE), ((0.0, inf, -10.0), NON_FINITE),
             ((0.0, 0.0, -inf), NON_FINITE), ((0.0, 0.0, nan), NON_FINITE)]
    if lens is not None:
        info = cam.info()
        # inside the lens: behind the front vertex (trace frame z < 0), and behind the sensor
        cases += [((0.01, 0.0, 0.05), BEHIND), ((0.0, 0.1, -info["originShift"] + 1.0), BEHIND)]
    pts = np.array([c[0] for c in cases], np.float32)
    scr, fl = _drive(driver, cam, p, pts)
    for (q, why), s2, f in zip(cases, scr, fl):
        assert f & 1 == 0 and _reason(f) == why, (q, hex(f))
        assert (s2.view(np.uint32) == 0).all(), (q, s2)
        sx, sy, g = cam.project_point(q)
        assert g == f and (sx, sy) == (0.0, 0.0)
    cam.close()


def test_model_none_and_outside_domain(driver):
    cam, p = _camera("tessar_f2.8.dat", lensModel=_capi.LENS_NONE)
    sx, sy, f = cam.project_point((0.1, 0.1, -10.0))
    assert f & 1 == 0 and _reason(f) == MODEL_NONE and (sx, sy) == (0.0, 0.0)
    cam.close()
    # a negative focal-length rescale (zoic.cpp:1651-1661): outside the geometric domain -- every point, the axis too
    cam, p = _camera("tessar_f2.8.dat", focalLength=-10.0)
    assert cam.info()["fastRunsStrict"]
    for q in ((0.1, 0.1, -10.0), (0.0, 0.0, -10.0)):
        sx, sy, f = cam.project_point(q)
        assert f & 1 == 0 and _reason(f) == OUTSIDE and (sx, sy) == (0.0, 0.0)
    scr, fl = _drive(driver, cam, p, np.array([[0.1, 0.1, -10.0]], np.float32))
    assert _reason(fl[0]) == OUTSIDE
    cam.close()


def test_clipped_and_lut_flags():
    cam, p = _camera("double_gauss_f2.0.dat")
    info = cam.info()
    L = Lens(info, p["sensorWidth"])
    seen = set()
    for t in np.linspace(0.05, 3.0, 60):   # from the axis out to far beyond the image circle, at 1 m
        sx, sy, f = cam.project_point((-t * 30.0, 0.0, -100.0))
        seen.add(f & 7)
        if f & 1 and np.hypot(sx, sy) * L.half_sensor * 8.0 > len(info["lutKeys"]) - 1:
            assert f & 4, (t, sx, hex(f))
    assert 1 in seen and any(v & 2 for v in seen), seen   # unclipped near the axis, clipped further out
    cam.close()


def test_reverse_ray_stays_false_unless_enabled():
    cam, p = _camera("tessar_f2.8.dat")
    lib = _capi.load()
    po = _capi.Vec3(0.5, -0.3, -100.0)
    ps = (ctypes.c_float * 2)(7.0, 8.0)
    t = ctypes.c_float(9.0)
    assert lib.zoic_camera_reverse_ray(cam._h, ctypes.byref(po), ctypes.c_float(0.5), ps, ctypes.byref(t)) == 0
    assert (ps[0], ps[1], t.value) == (7.0, 8.0, 9.0)   # untouched
    cam.set_reverse_projection(True)
    assert lib.zoic_camera_reverse_ray(cam._h, ctypes.byref(po), ctypes.c_float(0.5), ps, ctypes.byref(t)) == 1
    sx, sy, f = cam.project_point((0.5, -0.3, -100.0))
    assert f & 1 and (ps[0], ps[1]) == (np.float32(sx), np.float32(sy)) and t.value == 9.0
    assert cam.reverse_ray((0.5, -0.3, -100.0)) is True and cam.reverse_ray((0.5, -0.3, 100.0)) is False
    cam.set_reverse_projection(False)
    assert cam.reverse_ray((0.5, -0.3, -100.0)) is False
    cam.close()


def test_errors():
    lib = _capi.load()
    po = _capi.Vec3(0.1, 0.1, -10.0)
    ps = (ctypes.c_float * 2)()
    f = ctypes.c_uint32()
    assert lib.zoic_project_point(None, ctypes.byref(po), ps, ctypes.byref(f)) == 1
    assert lib.zoic_camera_set_reverse_projection(None, 1) == 1
    fresh = ZoicCamera(device=-1)
    with pytest.raises(ZoicError) as e:
        fresh.project_point((0.1, 0.1, -10.0))
    assert e.value.status_name == "ZOIC_ERR_NOT_UPDATED"
    assert lib.zoic_project_point(fresh._h, None, ps, None) == 1
    fresh.close()
    cam, p = _camera("tessar_f2.8.dat")
    assert lib.zoic_project_point(cam._h, ctypes.byref(po), ps, None) == 0   # flags may be NULL
    with pytest.raises(ZoicError) as e:   # a tables-only camera has no device
        cam.project_points(np.zeros((4, 3), np.float32))
    assert e.value.status_name == "ZOIC_ERR_NO_DEVICE"
    cam.close()


def test_host_latency():
    """zoic_project_point on one host thread: the median is reported (target <= 3 us on one core, C3 lens at focalDistance)"""
    cam, p = _camera("double_gauss_f2.0.dat", focalLength=5.0, fStop=2.0)
    pts, _, depth = kolb_point_set(cam.info(), p["sensorWidth"], p["focalDistance"], grid=16)
    pts = pts[depth == 1]
    lib = _capi.load()
    vec = [_capi.Vec3(*map(float, q)) for q in pts]
    ps = (ctypes.c_float * 2)()
    f = ctypes.c_uint32()
    fn, h = lib.zoic_project_point, cam._h
    t0 = time.perf_counter()
    for v in vec:
        fn(h, ctypes.byref(v), ps, ctypes.byref(f))
    per_call = (time.perf_counter() - t0) / len(vec)
    print("zoic_project_point through ctypes: %.2f us per call (ctypes adds ~1 us)" % (per_call * 1e6))
    assert per_call < 1e-3
    cam.close()

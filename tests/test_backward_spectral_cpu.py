"""The backward paths at a wavelength per item, without a GPU: the C-ABI declares and exports the four calls, the two gfx950 kernels
keep their budget, and the host builds (zoic_trace_back_ray_spectral, zoic_project_point_spectral on tables-only cameras)
  - equal the d-line calls bit for bit at 587.5618 nm,
  - agree with the f64 restatement written from the definition (backward_spectral_ref.py) at 400, 486.1327, 656.2725 and 700 nm as
    well as the d-line calls agree with theirs,
  - show lateral colour of the right size, and none for a prescription without V-numbers,
  - refuse a wavelength outside [360, 830] nm before anything else.

Accuracy.  Lenses: C2 (Tessar) and C5 (Petzval) with their files' V-numbers; C3 (double Gauss), C4 (fisheye) and the triplet with
V = 50 for every glass.  Trace-back inputs: the oracle's d-line records of weight > 0 on the 192 x 108 x 2 frame (generic rays: the f64
restatement is the judge); projection inputs: reverse_ref.kolb_point_set.  The bound is 2 x the d-line call's own figure
max |Ps(library) - Ps(f64)| on the same configuration and set, measured in the same test: the spectral ratio is a rounded quotient of
two rounded indices where the d-line table holds a rounded quotient of two exact ones, and the rays pass at slightly other heights.
Edge rays (TraceBack.edge: 1e-2 at the stop, 1e-4 elsewhere) are left out; their share is asserted <= 2 % from the restatement alone,
before the library is looked at.  Measured (max / p99 of |library - f64|, in units of 1e-7; d = the d-line call):

    trace-back       d           400 nm       486.1327     656.2725     700 nm       edge share (d / 400 / 486 / 656 / 700, %)
    C2 Tessar     7.6 / 4.1    8.2 / 4.4    8.9 / 5.1    7.8 / 4.0    8.0 / 4.2    0.45 / 0.03 / 0.30 / 0.51 / 0.53
    C3 dbl Gauss  9.0 / 5.3   10.2 / 5.1   10.7 / 6.3   10.3 / 5.1    8.6 / 4.8    0.01 / 0.01 / 0.01 / 0.01 / 0.02
    C4 fisheye    6.7 / 3.7    8.1 / 3.7    6.8 / 3.6    6.4 / 3.6    6.6 / 3.7    0.98 / 0.98 / 0.92 / 0.96 / 0.88
    C5 Petzval    3.2 / 1.6    2.6 / 1.7    2.6 / 1.6    3.4 / 2.1    2.8 / 1.6    0.31 / 0.05 / 0.25 / 0.33 / 0.38
    triplet       8.2 / 4.1    7.3 / 3.6    7.4 / 3.9    7.7 / 3.9    7.7 / 3.5    0.10 / 0.04 / 0.08 / 0.10 / 0.12

    projection       d           400 nm       486.1327     656.2725     700 nm
    C2 Tessar     5.3 / 3.8    5.1 / 3.5    4.7 / 3.5    4.9 / 3.5    5.1 / 3.6
    C3 dbl Gauss  5.0 / 3.2    5.8 / 3.7    5.6 / 3.1    5.0 / 3.2    5.2 / 3.7
    C4 fisheye   10.7 / 6.7    9.2 / 6.5    9.9 / 6.3   10.5 / 6.5    9.1 / 5.9
    C5 Petzval    1.6 / 1.4    2.0 / 1.3    2.1 / 1.3    2.2 / 1.8    1.6 / 1.4
    triplet       4.9 / 3.7    6.2 / 4.1    5.9 / 3.6    5.7 / 4.2    4.7 / 3.4

The f64 projection is backward_spectral_ref.chief_through: the chief ray through the stop's centre found by bracketing and bisection.
"""
import ctypes
import re

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera

import backward_spectral_ref as bs
import traceback_cases as tc
from library_facts import header_text, kernel_resources
from reverse_ref import kolb_point_set, thin_point_set
from traceback_cases import lib_project, lib_trace
from traceback_ref import CLIPPED, MISS, TIR

NEW = ("zoic_trace_back_rays_spectral_device", "zoic_trace_back_ray_spectral", "zoic_project_points_spectral_device",
       "zoic_project_point_spectral")
EDGE_CAP = 0.02
F32 = np.float32


def _camera(name, **over):
    p = dict(tc.params_of(name), **over)
    return tc.update(ZoicCamera(device=-1), p), p


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


_RECORDS = {}


def _records(oracle_lib, name):
    if name not in _RECORDS:
        _RECORDS[name] = tc.oracle_records(oracle_lib, tc.params_of(name))[1:]
    return _RECORDS[name]


_POINTS = {}


def _points(name):
    """the reverse projection's point set of a configuration (reverse_ref: points (m,3) f32, samples (m,2), depth index (m,))"""
    if name not in _POINTS:
        cam, p = _camera(name)
        info = cam.info()
        if name in tc.THIN:
            _POINTS[name] = thin_point_set(float(info["tan_fov"]), p["focalDistance"])
        else:
            _POINTS[name] = kolb_point_set(info, p["sensorWidth"], p["focalDistance"])
        cam.close()
    return _POINTS[name]


# ---- 1. symbols --------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_spectral_backward_calls():
    text = header_text()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"ZOIC_TRACE_BACK_WAVELENGTH\s*=\s*8\b", text) and re.search(r"ZOIC_PROJECT_WAVELENGTH\s*=\s*6\b", text)
    assert _capi.TRACE_BACK_WAVELENGTH == bs.TB_WAVELENGTH == 8 and _capi.PROJECT_WAVELENGTH == bs.PROJECT_WAVELENGTH == 6
    assert _capi.load().zoic_abi_version() == 5 and _capi.ABI_VERSION == 5


# ---- 2. bit identity at the d-line ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4", "C5", "triplet"])
def test_trace_back_at_the_d_line_is_the_d_line_call(oracle_lib, name):
    cam, p = _camera(name)
    bs.set_dispersion(cam, name)
    o, d = bs.trace_back_rays(tc, cam.info(), _records(oracle_lib, name), name in tc.KOLB)
    ps0, fl0 = lib_trace(cam, o, d)
    ps1, fl1 = lib_trace(cam, o, d, bs.LAMBDA_D)
    print("%s: %d rays, %d traced back, reasons %s" % (name, len(o), int((fl0 & 1).sum()), sorted(set(tc.reason(fl0[(fl0 & 1) == 0]).tolist()))))
    assert (fl0 & 1).sum() >= 1000 and ((fl0 & 1) == 0).sum() >= 100
    assert np.array_equal(fl0, fl1)
    assert _same_bits(ps0, ps1)
    sx, sy, f = cam.trace_back_ray(o[0], d[0], wavelength=bs.LAMBDA_D)   # the Python keyword reaches the same call
    assert _same_bits(np.array([sx, sy], F32), ps0[0]) and f == fl0[0]
    assert cam.trace_back_ray(o[0], d[0]) == (sx, sy, f)
    cam.close()


@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4", "C5", "triplet"])
def test_projection_at_the_d_line_is_the_d_line_call(name):
    cam, p = _camera(name)
    bs.set_dispersion(cam, name)
    pts = _points(name)[0]
    assert len(pts) >= 1000
    ps0, fl0 = lib_project(cam, pts)
    ps1, fl1 = lib_project(cam, pts, bs.LAMBDA_D)
    assert (fl0 & 1).mean() >= 0.99
    assert np.array_equal(fl0, fl1)
    assert _same_bits(ps0, ps1)
    sx, sy, f = cam.project_point(pts[0], wavelength=bs.LAMBDA_D)
    assert _same_bits(np.array([sx, sy], F32), ps0[0]) and f == fl0[0]
    assert cam.project_point(pts[0]) == (sx, sy, f)
    cam.close()


# ---- 3. accuracy against the f64 restatement -------------------------------------------------------------------------------------
def _tb_compare(T, cam, o, d, lam):
    """one wavelength (None: the d-line call and the d-line restatement).  Returns max and p99 of |library - f64| and the edge share."""
    ref = T.trace(o, d) if lam is None else T.trace_at(o, d, lam)
    edge = T.edge(ref)
    assert len(edge) >= 8192 and edge.mean() <= EDGE_CAP, (lam, edge.mean())   # the inputs, judged by the restatement alone
    ps, fl = lib_trace(cam, o, d, lam)
    ok = (fl & 1) == 1
    assert np.array_equal(ok[~edge], ref["traced"][~edge]), (lam, int((ok[~edge] != ref["traced"][~edge]).sum()))
    keep = ~T.decision_edge(ref)
    no = keep & ~ok
    assert np.array_equal(tc.reason(fl[no]), ref["reason"][no]), lam
    ended = no & np.isin(ref["reason"], (MISS, CLIPPED, TIR))
    assert np.array_equal(tc.iface(fl[ended]), ref["iface"][ended]), lam
    assert (ps[~ok].view(np.uint32) == 0).all()
    both = ~edge & ok & ref["traced"]
    # (a d-line record need not pass in another colour: the fisheye at 400 nm vignettes a fifth of them, in f64 and in the library alike)
    assert both.sum() >= 4096
    err = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
    return float(err.max()), float(np.percentile(err, 99)), float(edge.mean())


@pytest.mark.parametrize("name", list(bs.DISPERSIVE))
def test_trace_back_accuracy_at_four_wavelengths(oracle_lib, name):
    cam, p = _camera(name)
    bs.set_dispersion(cam, name)
    disp = cam.dispersion()
    assert disp["cauchy_b"].any()
    o, d, w = _records(oracle_lib, name)
    o, d = o[w > 0], d[w > 0]
    T = bs.SpectralTraceBack(cam.info(), p, disp)
    d_max, d_p99, d_edge = _tb_compare(T, cam, o, d, None)
    print("%s trace-back   d-line : max %.3g p99 %.3g edge %.2f %%" % (name, d_max, d_p99, 100 * d_edge))
    for lam in bs.LAMBDAS:
        e_max, e_p99, e_edge = _tb_compare(T, cam, o, d, lam)
        print("%s trace-back %8.4f : max %.3g p99 %.3g edge %.2f %%  (%.2f of the d-line max)" % (name, lam, e_max, e_p99, 100 * e_edge, e_max / d_max))
        assert e_max <= 2.0 * d_max, (lam, e_max, d_max)
    cam.close()


def _proj_compare(cam, p, pts, lam):
    info, disp = cam.info(), cam.dispersion()
    ref, ok_ref = bs.project_at(info, p["sensorWidth"], disp, pts, bs.LAMBDA_D if lam is None else lam)
    ps, fl = lib_project(cam, pts, lam)
    ok = (fl & 1) == 1
    assert ok_ref.mean() >= 0.99 and ok[ok_ref].all(), (lam, ok_ref.mean(), ok.mean())
    err = np.abs(ps.astype(np.float64) - ref).max(1)[ok & ok_ref]
    return float(err.max()), float(np.percentile(err, 99)), ps, ref, ok & ok_ref


@pytest.mark.parametrize("name", list(bs.DISPERSIVE))
def test_projection_accuracy_at_four_wavelengths(name):
    cam, p = _camera(name)
    bs.set_dispersion(cam, name)
    pts = _points(name)[0]
    d_max, d_p99 = _proj_compare(cam, p, pts, None)[:2]
    print("%s projection   d-line : max %.3g p99 %.3g (%d points)" % (name, d_max, d_p99, len(pts)))
    for lam in bs.LAMBDAS:
        e_max, e_p99 = _proj_compare(cam, p, pts, lam)[:2]
        print("%s projection %8.4f : max %.3g p99 %.3g  (%.2f of the d-line max)" % (name, lam, e_max, e_p99, e_max / d_max))
        assert e_max <= 2.0 * d_max, (lam, e_max, d_max)
    cam.close()


# ---- 4. the effect ---------------------------------------------------------------------------------------------------------------
def test_lateral_colour_of_the_tessar_is_there_and_the_right_size():
    """Off-axis points (|s| > 0.3) of the Tessar's set at focalDistance: Ps(F line) - Ps(C line) of the library equals the restatement's
    within item 3's bound (2 x the d-line figure of this set), and is itself more than 10 x that bound -- measured: the restatement's
    difference is 1.4e-4 ... 7.3e-4 over these points (file V-numbers), the bound 8.9e-7, |library - restatement| 6.3e-7."""
    cam, p = _camera("C2")
    pts, s, depth = _points("C2")
    pick = (depth == 1) & (np.hypot(s[:, 0], s[:, 1]) > 0.3)
    pts = pts[pick]
    assert len(pts) >= 256
    bound = 2.0 * _proj_compare(cam, p, pts, None)[0]
    _, _, psF, refF, okF = _proj_compare(cam, p, pts, 486.1327)
    _, _, psC, refC, okC = _proj_compare(cam, p, pts, 656.2725)
    ok = okF & okC
    lib_diff = (psF.astype(np.float64) - psC.astype(np.float64))[ok]
    ref_diff = (refF - refC)[ok]
    size = np.abs(ref_diff).max(1)
    print("lateral colour F - C: restatement %.3g ... %.3g, bound %.3g, |library - restatement| max %.3g" % (
        size.min(), size.max(), bound, np.abs(lib_diff - ref_diff).max()))
    assert size.min() > 10.0 * bound, (size.min(), bound)
    assert np.abs(lib_diff - ref_diff).max() <= bound
    cam.close()


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_a_prescription_without_v_numbers_has_no_colour(oracle_lib, name):
    """4-column files and no override: B = 0 everywhere, every valid wavelength gives the d-line bits"""
    cam, p = _camera(name)
    assert not cam.dispersion()["cauchy_b"].any()
    o, d, w = _records(oracle_lib, name)
    o, d = o[::16], d[::16]
    pts = _points(name)[0][::4]
    ps0, fl0 = lib_trace(cam, o, d)
    qs0, gl0 = lib_project(cam, pts)
    for lam in (360.0, 400.0, 656.2725, 830.0):
        ps1, fl1 = lib_trace(cam, o, d, lam)
        assert np.array_equal(fl0, fl1) and _same_bits(ps0, ps1), lam
        qs1, gl1 = lib_project(cam, pts, lam)
        assert np.array_equal(gl0, gl1) and _same_bits(qs0, qs1), lam
    cam.close()


# ---- 5. rejection ----------------------------------------------------------------------------------------------------------------
REJECT_CAMERAS = [("C2", {}), ("C1", {}), ("C1", dict(useDof=False)), ("C3", dict(lensModel=_capi.LENS_NONE)), ("C3", dict(focalLength=-10.0))]


@pytest.mark.parametrize("name,over", REJECT_CAMERAS)
def test_a_rejected_wavelength_is_reported_before_anything_else(name, over):
    cam, p = _camera(name, **over)
    ray = ((0.05, 0.02, -3.0), (0.01, -0.02, -1.0))
    point = (2.0, -1.0, -100.0)
    d_tb, d_pp = cam.trace_back_ray(*ray), cam.project_point(point)
    for lam in bs.REJECTED:
        for bad_ray in (ray, ((np.nan, 0.0, -1.0), (0.0, 0.0, -1.0)), (ray[0], (0.0, 0.0, 1.0))):   # (a rejected ray too: the wavelength comes first)
            sx, sy, f = cam.trace_back_ray(*bad_ray, wavelength=lam)
            assert f == _capi.TRACE_BACK_WAVELENGTH << 8, (lam, hex(f))
            assert np.array([sx, sy], F32).view(np.uint32).tolist() == [0, 0]
        for bad_point in (point, (np.nan, 0.0, -10.0), (0.1, 0.2, 1.0)):
            sx, sy, f = cam.project_point(bad_point, wavelength=lam)
            assert f == _capi.PROJECT_WAVELENGTH << 8, (lam, hex(f))
            assert np.array([sx, sy], F32).view(np.uint32).tolist() == [0, 0]
    for lam in (360.0, 830.0, 500.0):   # accepted: the ends of the range included
        tb, pp = cam.trace_back_ray(*ray, wavelength=lam), cam.project_point(point, wavelength=lam)
        assert tc.reason(tb[2]) != _capi.TRACE_BACK_WAVELENGTH and tc.reason(pp[2]) != _capi.PROJECT_WAVELENGTH
        assert (tb[2] & 1) == (d_tb[2] & 1) and (pp[2] & 1) == (d_pp[2] & 1)
        if name == "C1" or over:   # THINLENS, NONE, outside the domain: the d-line answer, whatever the wavelength
            assert tb == d_tb and pp == d_pp, (lam, tb, d_tb, pp, d_pp)
    cam.close()


def test_mixed_wavelengths_follow_the_restatement(oracle_lib):
    """valid and rejected wavelengths interleaved over one ray set: the decisions and reasons of the restatement"""
    cam, p = _camera("C2")
    o, d, w = _records(oracle_lib, "C2")
    o, d = o[w > 0][:2048], d[w > 0][:2048]
    lam = bs.mixed_wavelengths(len(o))
    ok_lam = bs.valid(lam)
    lam_few = lam.copy()
    lam_few[ok_lam] = np.asarray(bs.LAMBDAS, F32)[np.arange(int(ok_lam.sum())) % 4]   # (the restatement runs one pass per distinct wavelength)
    T = bs.SpectralTraceBack(cam.info(), p, cam.dispersion())
    ref = T.trace_at(o, d, lam_few)
    ps, fl = lib_trace(cam, o, d, lam_few)
    assert (tc.reason(fl[~ok_lam]) == bs.TB_WAVELENGTH).all() and (fl[~ok_lam] & 1 == 0).all() and (ps[~ok_lam].view(np.uint32) == 0).all()
    assert (ref["reason"][~ok_lam] == bs.TB_WAVELENGTH).all()
    keep = ok_lam & ~T.edge(ref)
    assert np.array_equal((fl[keep] & 1) == 1, ref["traced"][keep])
    cam.close()


# ---- 6. budget -------------------------------------------------------------------------------------------------------------------
def test_spectral_backward_kernels_budget():
    res = kernel_resources()
    for kernel in ("trace_back_spectral_kernel", "project_points_spectral_kernel"):
        hit = {k: v for k, v in res.items() if kernel in k}
        assert len(hit) == 1, (kernel, sorted(res))
        for k, v in hit.items():
            print(k, v)
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] == 0, (k, v)
            assert v["vgpr"] <= 64 and v["agpr"] == 0, (k, v)


# ---- the control of the GPU round trip, judged by the restatement ----------------------------------------------------------------
def test_d_line_trace_back_of_coloured_rays_misses_by_more_than_the_round_trip_bound(oracle_lib):
    """tests/test_backward_spectral_gpu.py relies on this separation on C2: over wavelengths uniform in [400, 700] nm, the sample a ray
    lands on at its own wavelength and the one the d-line trace gives it differ, in the median, by far more than the spectral round
    trip may err (2 x the d-line round trip's maximum; DESIGN 4.10: 1.4e-6 ... 1.9e-6, so at most ~4e-6).  f64 restatement only, on
    the oracle's d-line records (the same lines through the same glass).  Measured: median 2.9e-4, 10 % quantile 4.8e-5."""
    cam, p = _camera("C2")
    o, d, w = _records(oracle_lib, "C2")
    o, d = o[w > 0][::4], d[w > 0][::4]
    T = bs.SpectralTraceBack(cam.info(), p, cam.dispersion())
    lam = np.round(np.random.default_rng(5).uniform(400.0, 700.0, len(o)) / 10.0).astype(F32) * F32(10.0)   # a 31-value grid: 31 passes
    at_lam, at_d = T.trace_at(o, d, lam), T.trace(o, d)
    both = at_lam["traced"] & at_d["traced"]
    shift = np.abs(at_lam["ps"] - at_d["ps"]).max(1)[both]
    print("C2: |Ps(lambda) - Ps(d)| median %.3g, 10 %% quantile %.3g, max %.3g over %d rays" % (np.median(shift), np.percentile(shift, 10), shift.max(), both.sum()))
    assert np.median(shift) > 5.0 * 4e-6
    cam.close()

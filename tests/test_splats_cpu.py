"""Lens splats without a GPU: the C-ABI declares and exports the four calls, the gfx950 kernels keep their budget, and the host twin
-- csrc/splat.hpp compiled here with clang++ (splat_driver.py) and the library's zoic_splat_point / zoic_splat_point_spectral on a
tables-only camera -- gives the records of an independent restatement (splat_ref.py: aims and rays from pupil_rays, each ray traced
by the pinned zoic_trace_back_ray_jacobian, the measures in numpy float32) bit for bit, all 32 bytes; the measures agree with f64
within bounds derived from their operation counts; and the exact properties of the definition hold.

Cameras and points: pupil_cases.py (six cameras, ten points); bounds from the host pupil bounds at lattice 16; m in {1, 5, 64}."""
import ctypes
import functools
import re

import numpy as np
import pytest

from zoic_amd import ZoicCamera, _capi, solid_angle_measure, splat_records

import backward_spectral_ref as bs
import host_drivers
import pupil_cases as pc
import pupil_driver
import splat_driver
import splat_ref
import traceback_cases as tc
from library_facts import header_text, kernel_resources
from traceback_ref import AWAY, MODEL, NON_FINITE, OUTSIDE_DOMAIN

NEW = ("zoic_splat_points_device", "zoic_splat_points_spectral_device", "zoic_splat_point", "zoic_splat_point_spectral")
AIMS = (1, 5, 64)
G = 16
F32 = np.float32
U = 2.0 ** -24                                    # the unit roundoff of f32
BELOW_ONE = F32(1.0) - F32(2.0 ** -24)            # the largest float below 1


def _u(n, m, seed=21):
    """(n,m,2) float32 in [0,1); where there is room, the first aim of point 0 is u = 0 and that of point 1 the largest float below 1"""
    u = np.random.default_rng(seed + m).random((n, m, 2)).astype(F32)
    u[0, 0] = 0.0
    u[1, 0] = BELOW_ONE
    return u


@functools.lru_cache(maxsize=None)
def _camera(name, dispersive=False):
    p = pc.params_of(name)
    cam = tc.update(ZoicCamera(device=-1), p)
    if dispersive and pc.CAMERAS[name][0] in bs.DISPERSIVE:
        bs.set_dispersion(cam, pc.CAMERAS[name][0])
    return cam, p


@functools.lru_cache(maxsize=None)
def _bounds(name, spectral=False):
    """the host pupil bounds of the camera's ten points at lattice 16 (read only)"""
    cam, p = _camera(name, spectral)
    pts = pc.points(p)
    lam = pc.wavelengths(len(pts)) if spectral else None
    b = pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, G, None, lam, cam.dispersion() if spectral else None)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _reference(name, m, spectral=False, dline_bounds=False):
    """(records (10, m), dirs, J) of the restatement (computed once, shared, read only)"""
    cam, p = _camera(name, spectral)
    pts = pc.points(p)
    b = _bounds(name, spectral and not dline_bounds)
    ref = splat_ref.reference(cam, pts, b, _u(len(pts), m), pc.wavelengths(len(pts)) if spectral else None)
    for a in ref:
        a.setflags(write=False)
    return ref


def _lib_records(cam, pts, b, u, lam=None):
    """zoic_splat_point / _spectral on every point, as (n, m) records"""
    return np.stack([cam.splat_point(pts[i], b[i:i + 1], u[i], None if lam is None else lam[i]) for i in range(len(pts))])


def _reason(flags):
    return (np.asarray(flags).astype(np.int64) >> 8) & 15


def test_abi_declares_and_exports_the_calls():
    text = header_text()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert _capi.load().zoic_abi_version() == 5
    assert ctypes.sizeof(_capi.Splat) == 32 == np.dtype(_capi.SPLAT_DTYPE).itemsize
    assert [f[0] for f in _capi.Splat._fields_] == [f[0] for f in _capi.SPLAT_DTYPE] == ["sx", "sy", "ax", "ay", "area", "angle", "flags", "reserved"]
    assert re.search(r"#define\s+ZOIC_SPLAT_NO_BOX\s+0x1000u", text) and _capi.SPLAT_NO_BOX == 0x1000 == splat_ref.NO_BOX
    # the bit is free in the trace-back's flag word: bit 0, bit 2, the reason in bits 8-11, the interface in bits 16-21
    assert re.search(r"#define\s+ZOIC_TRACE_BACK_REASON\(flags\)\s+\(\(\(flags\)\s*>>\s*8\)\s*&\s*0xFu\)", text)
    assert re.search(r"#define\s+ZOIC_TRACE_BACK_INTERFACE\(flags\)\s+\(\(\(flags\)\s*>>\s*16\)\s*&\s*0x3Fu\)", text)
    assert (0x1 | 0x4 | (0xF << 8) | (0x3F << 16)) & _capi.SPLAT_NO_BOX == 0


def test_kernel_budget():
    res = {k: v for k, v in kernel_resources().items() if "splat" in k}
    assert len(res) == 6, sorted(res)   # d-line and spectral, an instance per lens model
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)


@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_host_twin_equals_the_restatement_bitwise(name):
    cam, p = _camera(name)
    pts, b = pc.points(p), _bounds(name)
    traced = 0
    for m in AIMS:
        ref, _, _ = _reference(name, m)
        u = _u(len(pts), m)
        got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u)
        assert splat_ref.same_records(got, ref), (m, splat_ref.differing(got, ref))
        lib = _lib_records(cam, pts, b, u)
        assert splat_ref.same_records(lib, ref), (m, splat_ref.differing(lib, ref))
        assert (ref["reserved"] == 0).all()
        traced += int((ref["flags"] & 1).sum())
    assert traced >= 70   # the cases are not all refused


@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_spectral_host_twin_equals_the_restatement_bitwise(name):
    """with the bounds of the spectral pupil-bounds call (the point with the invalid wavelength has an empty box), and, m = 5, with
    the d-line bounds, so that the invalid wavelength reaches the trace"""
    cam, p = _camera(name, True)
    pts = pc.points(p)
    lam, disp = pc.wavelengths(len(pts)), cam.dispersion()
    bad = lam == F32(pc.BAD_LAMBDA)
    assert bad.sum() == 1
    for m, dline_bounds in [(m, False) for m in AIMS] + [(5, True)]:
        b = _bounds(name, not dline_bounds)
        ref, _, _ = _reference(name, m, True, dline_bounds)
        u = _u(len(pts), m)
        got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u, lam, disp)
        assert splat_ref.same_records(got, ref), (m, dline_bounds, splat_ref.differing(got, ref))
        lib = _lib_records(cam, pts, b, u, lam)
        assert splat_ref.same_records(lib, ref), (m, dline_bounds, splat_ref.differing(lib, ref))
        if dline_bounds:   # a box, but no wavelength: refused by the trace, the aim is written, the measures are not
            r = ref[bad]
            assert (b["count"][bad] > 0).all() or name == "C5"   # (C5 sees nothing from that point at the d-line either)
            if (b["count"][bad] > 0).all():
                assert (r["flags"] == bs.TB_WAVELENGTH << 8).all() and (r["ax"] != 0).all()
                assert not r["area"].view(np.uint32).any() and not r["angle"].view(np.uint32).any()
        else:
            assert (ref[bad]["flags"] == splat_ref.NO_BOX).all()
        # at the d-line the spectral call is the d-line call
        dline = np.full(len(pts), bs.LAMBDA_D, F32)
        assert splat_ref.same_records(splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u, dline, disp),
                                      splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u))
    if p["lensModel"] == _capi.RAYTRACED:   # the glass disperses: some record moves with the wavelength
        assert not splat_ref.same_records(_reference(name, 64, True, True)[0], _reference(name, 64)[0])


@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_screen_sample_and_flags_are_the_trace_backs(name):
    """sx, sy and the flag word equal zoic_trace_back_ray's (spectral: zoic_trace_back_ray_spectral's) for the same ray, bit for bit"""
    cam, p = _camera(name)
    pts, b = pc.points(p), _bounds(name)
    m = 64
    u = _u(len(pts), m)
    got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u).reshape(-1)
    _, o, d, empty = splat_ref.aims_and_rays(pts, b, u, cam.pupil_square()[0])
    ps, fl = tc.lib_trace(cam, o[~empty], d[~empty])
    assert np.array_equal(got["flags"][~empty], fl)
    assert np.array_equal(got["sx"][~empty].view(np.uint32), ps[:, 0].view(np.uint32))
    assert np.array_equal(got["sy"][~empty].view(np.uint32), ps[:, 1].view(np.uint32))
    scam, _ = _camera(name, True)
    lam = pc.wavelengths(len(pts))
    sgot = splat_driver.drive_splat(splat_driver.splat(), scam, p, pts, b, u, lam, scam.dispersion()).reshape(-1)
    ps, fl = tc.lib_trace(scam, o[~empty], d[~empty], np.repeat(lam, m)[~empty])
    assert np.array_equal(sgot["flags"][~empty], fl)
    assert np.array_equal(sgot["sx"][~empty].view(np.uint32), ps[:, 0].view(np.uint32))
    assert np.array_equal(sgot["sy"][~empty].view(np.uint32), ps[:, 1].view(np.uint32))


@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_measures_against_f64(name):
    """area: the f64 determinant of the f32 J entries, within 3 u (|J3 J10| + |J4 J9|), u = 2^-24: two products and one difference,
    each correctly rounded (u |J3 J10| + u |J4 J9| + u |difference| <= 2 u (...), to first order).
    angle: the f64 value of area r^3 / dz from the record's f32 area and the f32 dir, within the relative 8 u the definition's issue
    sets.  Recount of the operations as splat.hpp writes them: NINE rounded operations -- three products and two sums in r2, one
    root, the product r2 r, the product area (r2 r), the quotient.  To first order r2 carries at most 3 u (a product and two sums on
    its longest path), r = sqrt(r2) 1.5 u + u, r2 r 3 u + 2.5 u + u = 6.5 u, the numerator 7.5 u, the quotient 8.5 u: the worst
    case of nine same-signed half-ulp errors lies half a unit above the asserted 8 u, the sums of positive terms never reach it
    together, and the largest figure seen is printed (2.4 to 3.0 u per camera on these cases).
    angle against solid_angle_measure(J, dir): equal signs on every traced ray; the largest relative difference is printed, not
    asserted (it measures how well J_d . dir = 0 holds in f32)."""
    cam, p = _camera(name)
    worst_area = worst_angle = worst_measure = 0.0
    n = 0
    for m in AIMS:
        ref, d, J = _reference(name, m)
        r = ref.reshape(-1)
        t = (r["flags"] & 1) == 1
        r, d64, J64 = r[t], d[t].astype(np.float64), J[t].astype(np.float64)
        n += len(r)
        p0, p1 = J64[:, 3] * J64[:, 10], J64[:, 4] * J64[:, 9]
        err = np.abs(r["area"].astype(np.float64) - (p0 - p1))
        tol = 3.0 * U * (np.abs(p0) + np.abs(p1))
        assert (err <= tol).all(), (m, float((err / tol).max()))
        worst_area = max(worst_area, float((err / np.maximum(tol, 1e-300)).max()))
        r3 = (d64 * d64).sum(1) ** 1.5
        exact = r["area"].astype(np.float64) * r3 / d64[:, 2]
        assert np.isfinite(exact).all() and (exact != 0).any()
        err = np.abs(r["angle"].astype(np.float64) - exact)               # (a thin lens in focus has area = angle = 0 exactly)
        rel = err[exact != 0] / np.abs(exact[exact != 0])
        print("%s m=%d: angle against f64, largest relative error %.2f u" % (name, m, float(rel.max()) / U))
        assert (err <= 8.0 * U * np.abs(exact)).all(), (m, float(rel.max()) / U)
        worst_angle = max(worst_angle, float(rel.max()) / U)
        sam = solid_angle_measure(J[t].reshape(-1, 2, 6), d[t])
        assert np.array_equal(np.sign(sam), np.sign(r["angle"].astype(np.float64))), m
        nz = sam != 0
        worst_measure = max(worst_measure, float((np.abs(sam - r["angle"])[nz] / np.abs(sam[nz])).max()))
    assert n >= 70
    print("%s: %d traced; area error %.2f of its bound; angle %.2f u; angle against solid_angle_measure %.3g relative"
          % (name, n, worst_area, worst_angle, worst_measure))


@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_exact_properties(name):
    cam, p = _camera(name)
    pts, b = pc.points(p), _bounds(name)
    none = b["count"] == 0
    assert none[pc.BEHIND] and none[pc.NON_FINITE] and not none[:3].any()   # (the on-axis points always see the lens)
    lo, hi = b["aim"][:, None, 0:2], b["aim"][:, None, 2:4]
    for m in AIMS:
        ref, _, _ = _reference(name, m)
        # every aim lies inside its box, at u = 0 and at the largest float below 1 too
        a = np.stack([ref["ax"], ref["ay"]], 2)
        assert ((a >= lo) & (a <= hi))[~none].all()
        assert np.array_equal(a[0, 0].view(np.uint32), b["aim"][0, 0:2].view(np.uint32))          # u = 0: the box's lower corner
        assert (a[1, 0] <= b["aim"][1, 2:4]).all() and (a[1, 0] > b["aim"][1, 0:2]).all()
        # an empty box: kSpNoBox, and 32 zero bytes apart from the flag
        e = ref[none].copy()
        assert (e["flags"] == splat_ref.NO_BOX).all()
        e["flags"] = 0
        assert not np.frombuffer(e.tobytes(), np.uint8).any()
        # a traced ray has its measures, a refused one has +0; no flag word of a traced or refused ray carries bit 12
        r = ref[~none]
        t = (r["flags"] & 1) == 1
        assert ((r["flags"] & splat_ref.NO_BOX) == 0).all()
        assert np.array_equal(np.sign(r["angle"][t]), -np.sign(r["area"][t]))                     # dz < 0 (a thin lens in focus: both 0)
        assert (r["area"][t] != 0).any()
        for k in ("sx", "sy", "area", "angle"):
            assert not r[k][~t].view(np.uint32).any(), k
        assert (_reason(r["flags"][~t]) != 0).all()


def test_u_outside_the_unit_square_and_nan_u():
    for name in ("C3", "C1"):
        cam, p = _camera(name)
        pts, b = pc.points(p)[:pc.BEHIND], _bounds(name)[:pc.BEHIND]
        n = len(pts)
        u = np.zeros((n, 6, 2), F32)
        u[:, 0] = (-0.5, 1.5)
        u[:, 1] = (2.0, -3.0)
        u[:, 2] = (np.nan, 0.5)
        u[:, 3] = (0.5, np.nan)
        u[:, 4] = (np.inf, -np.inf)
        u[:, 5] = (0.25, 0.75)
        got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u)
        bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
        assert np.array_equal(bits(got["ax"][:, 0]), bits(b["aim"][:, 0])) and np.array_equal(bits(got["ay"][:, 0]), bits(b["aim"][:, 3]))
        assert np.array_equal(bits(got["ax"][:, 1]), bits(b["aim"][:, 2])) and np.array_equal(bits(got["ay"][:, 1]), bits(b["aim"][:, 1]))
        assert np.array_equal(bits(got["ax"][:, 4]), bits(b["aim"][:, 2])) and np.array_equal(bits(got["ay"][:, 4]), bits(b["aim"][:, 1]))
        for k, nan_field in ((2, "ax"), (3, "ay")):
            r = got[:, k]
            assert (bits(r[nan_field]) == 0x7FC00000).all()
            assert (r["flags"] == NON_FINITE << 8).all()
            for f in ("sx", "sy", "area", "angle"):
                assert not bits(r[f]).any()
        assert ((got["flags"][:, 5] & 1) == 1).any()
        assert splat_ref.same_records(got, splat_ref.reference(cam, pts, b, u)[0])
        assert splat_ref.same_records(_lib_records(cam, pts, b, u), got)


def test_wholesale_refusals():
    """lensModel NONE, a pinhole thin lens and a camera outside the domain: their own pupil bounds are empty, so every splat is
    kSpNoBox; given a box all the same, the trace refuses the ray for the model's reason, the aim is written and the measures are not.
    Likewise a point behind the cap and a non-finite point."""
    base, thin = pc.params_of("C3"), pc.params_of("C1")
    pts = pc.points(base)
    u = _u(len(pts), 5)
    box = np.zeros(len(pts), _capi.PUPIL_BOUNDS_DTYPE)
    box["aim"], box["count"], box["lattice"], box["flags"] = (-0.5, -0.25, 0.5, 0.25), 7, 256, 1
    cases = [(dict(thin, useDof=False), MODEL), (dict(base, lensModel=_capi.LENS_NONE), MODEL), (dict(base, focalLength=-10.0), OUTSIDE_DOMAIN),
             (base, None), (thin, None)]
    for p, why in cases:
        cam = tc.update(ZoicCamera(device=-1), p)
        own = pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, G)
        got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, own, u)
        if why is not None:
            assert (own["count"] == 0).all() and (got["flags"] == splat_ref.NO_BOX).all()
        assert (got["flags"][[pc.BEHIND, pc.NON_FINITE]] == splat_ref.NO_BOX).all()
        forced = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, box, u)
        assert splat_ref.same_records(_lib_records(cam, pts, box, u), forced)
        rows = slice(None) if why is not None else [pc.BEHIND, pc.NON_FINITE]
        r = forced[rows]
        if why is not None:
            assert (r["flags"] == why << 8).all()
        else:
            assert (_reason(r["flags"][0]) == AWAY).all() and (r["flags"][1] == NON_FINITE << 8).all()
        assert ((r["ax"] >= -0.5) & (r["ax"] <= 0.5) & (r["ay"] >= -0.25) & (r["ay"] <= 0.25)).all() and (r["ax"] != 0).any()
        for f in ("sx", "sy", "area", "angle", "reserved"):
            assert not np.ascontiguousarray(r[f]).view(np.uint32).any(), f
        # a record with aims but bit 0 clear, or with bit 0 set but no count, is an empty box too
        for count, flags in ((7, 1 << 19), (0, 1)):
            odd = box.copy()
            odd["count"], odd["flags"] = count, flags
            assert (splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, odd, u)["flags"] == splat_ref.NO_BOX).all()
        cam.close()


def test_argument_errors_of_the_host_calls():
    lib = _capi.load()
    cam, p = _camera("C3")
    po = _capi.Vec3(0.0, 0.0, -100.0)
    b = _capi.PupilBounds.from_buffer_copy(_bounds("C3")[0:1].tobytes())
    assert b.count > 0
    m = 4
    u = _u(2, m)[1].copy()
    out = np.full(8 * m + 2, 7.0, F32)
    sentinel = out.tobytes()
    d, s = lib.zoic_splat_point, lib.zoic_splat_point_spectral
    B, O, Uu = ctypes.byref(b), out.ctypes.data, u.ctypes.data
    assert d(cam._h, ctypes.byref(po), B, 0, Uu, O) == 1                         # m = 0
    assert s(cam._h, ctypes.byref(po), B, 550.0, 0, Uu, O) == 1
    assert d(None, ctypes.byref(po), B, m, Uu, O) == 1
    assert d(cam._h, None, B, m, Uu, O) == 1
    assert d(cam._h, ctypes.byref(po), None, m, Uu, O) == 1
    assert d(cam._h, ctypes.byref(po), B, m, None, O) == 1
    assert d(cam._h, ctypes.byref(po), B, m, Uu, None) == 1
    assert d(cam._h, ctypes.byref(po), B, m, Uu, O + 2) == 1                     # misaligned output
    assert d(cam._h, ctypes.byref(po), B, m, Uu + 1, O) == 1                     # misaligned u
    assert s(cam._h, None, B, 550.0, m, Uu, O) == 1
    assert s(cam._h, ctypes.byref(po), None, 550.0, m, Uu, O) == 1
    assert s(cam._h, ctypes.byref(po), B, 550.0, m, None, O) == 1
    assert s(cam._h, ctypes.byref(po), B, 550.0, m, Uu, None) == 1
    assert s(cam._h, ctypes.byref(po), B, 550.0, m, Uu, O + 2) == 1
    fresh = ZoicCamera(device=-1)
    assert d(fresh._h, ctypes.byref(po), B, m, Uu, O) == 9                       # NOT_UPDATED
    assert s(fresh._h, ctypes.byref(po), B, 550.0, m, Uu, O) == 9
    fresh.close()
    assert out.tobytes() == sentinel                                             # nothing was written
    assert lib.zoic_splat_points_device(cam._h, 4, None, None, 1, None, None, None) == 11   # a tables-only camera: NO_DEVICE
    assert lib.zoic_splat_points_device(cam._h, 4, None, None, 0, None, None, None) == 1    # m = 0 with n > 0
    assert d(cam._h, ctypes.byref(po), B, m, Uu, O + 4) == 0                     # the records' own 4-byte alignment is enough
    assert (out[0] == 7.0) and (out[-1] == 7.0)                                  # and nothing is written past m records
    rec = splat_records(out[1:-1].reshape(m, 8).copy())
    assert rec.shape == (m,) and (rec["reserved"] == 0).all() and ((rec["flags"] & 1) == 1).any()
    assert splat_ref.same_records(rec, cam.splat_point((0.0, 0.0, -100.0), _bounds("C3")[0:1], u))
    with pytest.raises(ValueError):
        cam.splat_point((0.0, 0.0, -100.0), _bounds("C3")[0:2], u)


def test_python_wrappers():
    cam, p = _camera("C3")
    pts, b = pc.points(p), _bounds("C3")
    u = _u(len(pts), 5)
    ref, _, _ = _reference("C3", 5)
    # the dict of pupil_bounds_point, a structured record and its 12 floats are the same bounds
    as_dict = cam.pupil_bounds_point(pts[3], G)
    flat = np.ascontiguousarray(b[3:4]).view(F32).reshape(1, 12)
    for bounds in (as_dict, b[3:4], flat):
        assert splat_ref.same_records(cam.splat_point(pts[3], bounds, u[3]), ref[3])
    assert splat_ref.same_records(cam.splat_point(pts[3], as_dict, u[3], wavelength=bs.LAMBDA_D), ref[3])
    # splat_records: (n,m,8) float32 <-> (n,m) records
    f = np.ascontiguousarray(ref).view(F32).reshape(len(pts), 5, 8)
    assert splat_ref.same_records(splat_records(f), ref) and splat_records(ref) is not None
    with pytest.raises(ValueError):
        splat_records(np.zeros((3, 7), F32))
    with pytest.raises(ValueError):
        cam.splat_point(pts[3], as_dict, np.zeros((4, 3), F32))


def test_traced_share_on_the_stopped_down_camera():
    """C3 at f/8, the ten points, 256 uniform u each: the number of traced splats EQUALS the number pupil_rays + the trace-back give
    on the same u (tests/test_pupil_bounds_cpu.py holds that share against draws from the whole front square): the fused call loses
    none of what the box buys."""
    cam, p = _camera("C3-f8")
    pts, b = pc.points(p), _bounds("C3-f8")
    m = 256
    u = _u(len(pts), m, seed=9)
    got = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, b, u)
    _, o, d, _ = splat_ref.aims_and_rays(pts, b, u, cam.pupil_square()[0])
    fl = host_drivers.drive_traceback(host_drivers.traceback(), cam, p, o, d)[1]
    chain = ((fl & 1) == 1).reshape(len(pts), m) & (b["count"] > 0)[:, None]
    fused = (got["flags"] & 1) == 1
    print("traced: %d of %d splats (%.4f of those with a box)" % (fused.sum(), fused.size, fused[:pc.BEHIND].mean()))
    assert np.array_equal(fused, chain) and fused.sum() == chain.sum() > 0

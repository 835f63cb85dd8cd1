"""The trace-back Jacobian without a GPU: the C-ABI declares and exports the four calls, the two gfx950 kernels keep their budget, and
the host build of csrc/traceback_jacobian.hpp (zoic_trace_back_ray_jacobian on a tables-only camera) gives zoic_trace_back_ray's Ps and
flags bit for bit, J = 0 where nothing is traced, and a J that beats what a caller could do before: the f32 central-difference
Jacobian from the existing zoic_trace_back_ray.

Rays.  The oracle's forward records of traceback_cases' frame (192 x 108 x 2), dir normalised in f64 before the cast to f32.  For the
accuracy tests the start point is moved one front housing radius (THINLENS: one apertureRadius) out along the ray -- the same line.
A forward record's own origin lies ON the front element's cap, and trace_back_ray refuses a start point more than 2^-14 of the
housing radius behind that cap (kTbAway): the finite-difference neighbours origin - h s_o e_z would all be refused and the
yardstick would not exist.  A light tracer's origin is a scene point in front of the lens.  The bitwise tests use the records as
they are.

Errors are per ray |(J - Jref) S|_F / |Jref S|_F (traceback_jacobian_ref.py).  The ray set of a configuration: every 16th live record
(every 8th, 4th ... where that gives fewer than 1024 rays to keep: C5 has 8 722 live records) that the f64 trace takes back, outside
T.edge, with all 12 neighbours traced at the yardstick's step h s_i by the f64 trace and by the library.  The yardstick's step is the
h of 2^-6 ... 2^-14 with the lowest median error among those that leave out at most 3 % of the live rays picked (the neighbour
condition at a large step removes the rays that pass within h s_o of a housing: the range is narrowed from the top, the cap stays).
Measured (host build; J, then the yardstick at its step, then the yardstick's best median over ALL nine steps, which J is held to as
well):

    configuration     rays    J median / p99       yardstick h, median / p99      best median of any h
    C2 (Tessar)          2064    1.18e-7 / 3.17e-7    2^-9   1.22e-5 / 2.72e-5       5.36e-6 (2^-7)
    C3 (dbl. Gauss)      2544    2.57e-7 / 7.44e-7    2^-8   1.95e-5 / 4.08e-5       1.95e-5 (2^-8)
    C4 (fisheye)         2524    4.89e-6 / 1.86e-5    2^-12  6.59e-4 / 1.49e-3       1.67e-4 (2^-10)
    C5 (Petzval)         1070    1.52e-7 / 3.91e-7    2^-10  2.24e-5 / 4.79e-5       6.92e-6 (2^-8)      (every 8th live record)
    triplet f/2.5        1957    1.55e-7 / 4.19e-7    2^-9   1.11e-5 / 2.74e-5       8.77e-6 (2^-8)
    C1 (thin lens)       2563    6.73e-8 / 1.70e-7    2^-8   2.87e-6 / 8.19e-6       2.87e-6 (2^-8)
    C1 + vignetting      1228    6.47e-8 / 1.63e-7    2^-10  5.29e-6 / 1.38e-5       1.82e-6 (2^-8)
    C2 spectral          2066    1.32e-7 / 3.75e-7    2^-9   1.20e-5 / 2.68e-5       5.34e-6 (2^-7)
    C3 spectral          2549    2.25e-7 / 6.77e-7    2^-8   1.95e-5 / 4.24e-5       1.95e-5 (2^-8)
    triplet spectral     1924    1.31e-7 / 3.70e-7    2^-8   8.92e-6 / 1.62e-5       8.92e-6 (2^-8)

Jref at the steps 1e-5 s and 1e-6 s agrees to 9e-9 (C4) and 5e-10 or better elsewhere; |J_o dir| <= 6e-10 and |J_d dir| <= 1.3e-7 of
|J S|_F; the thin lens's entries are within 3.9 ulp of their row's largest.

The requirement: J's median <= the yardstick's / 4, J's p99 <= the yardstick's."""
import ctypes
import re

import numpy as np
import pytest

from zoic_amd import _capi, solid_angle_measure
from zoic_amd.camera import ZoicCamera
from zoic_amd.workloads import camera_params

import backward_spectral_ref as bs
import traceback_cases as tc
import traceback_jacobian_ref as jr
from library_facts import header_text, kernel_resources
from traceback_jacobian_ref import LAMBDA_D, LEFT_OUT_CAP, MIN_RAYS, best as _best, check_accuracy as _check_accuracy
from traceback_ref import RAYTRACED, TraceBack

NEW = ("zoic_trace_back_jacobian_device", "zoic_trace_back_ray_jacobian", "zoic_trace_back_jacobian_spectral_device",
       "zoic_trace_back_ray_jacobian_spectral")
SPECTRAL = ("C2", "C3", "triplet")
# the edge rows of test_traceback_gpu.py (origin, dir)
EDGE_ROWS = np.array([[0, 0, -1, 0, 0, -1], [0, 0, -1e30, 0, 0, -1e-30], [1e30, 0, -1, 0, 0, -1], [0, 0, -1, 1e30, 0, -1e-30],
                      [0, 0, 0, 0, 0, -1], [-0.0, -0.0, -0.0, -0.0, -0.0, -1], [0, 0, -1, 1, 0, -1e-38], [1e-30, 1e-30, -1e-30, 1e-30, 0, -1e-30]],
                     np.float32)


def _camera(p, name=None, spectral=False):
    cam = tc.update(ZoicCamera(device=-1), p)
    if spectral:
        bs.set_dispersion(cam, name)
    return cam


_RECORDS = {}


def records(oracle_lib, name):
    """(params, origin (N,3) f32, dir (N,3) f32 normalised in f64, weight (N,)) of the frame"""
    if name not in _RECORDS:
        p = tc.params_of(name)
        _, o, d, w = tc.oracle_records(oracle_lib, p)
        _RECORDS[name] = (p, np.ascontiguousarray(o, np.float32), jr.unit_f32(d), w)
    return _RECORDS[name]


def ray_sets(info, p, o, d, w):
    """every set the bitwise comparison runs on, concatenated"""
    O, D = [o, EDGE_ROWS[:, :3]], [d, EDGE_ROWS[:, 3:]]
    nf = tc.non_finite_rays()
    O.append(nf[0]); D.append(nf[1])
    rl = tc.random_lines(info, 4096)
    O.append(rl[0]); D.append(rl[1])
    if int(p["lensModel"]) == RAYTRACED:
        live = np.flatnonzero(w > 0)[::16]
        for fo, fd in tc.rejection_families(info, o[live], d[live]).values():
            O.append(fo); D.append(fd)
    return np.ascontiguousarray(np.concatenate(O), np.float32), np.ascontiguousarray(np.concatenate(D), np.float32)


def test_abi_declares_and_exports_the_jacobian_calls():
    text = header_text()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert _capi.load().zoic_abi_version() == 5


def test_jacobian_kernel_budget():
    res = {k: v for k, v in kernel_resources().items() if "trace_back_jacobian" in k}
    assert any("trace_back_jacobian_kernel" in k for k in res) and any("trace_back_jacobian_spectral_kernel" in k for k in res), list(res)
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr_spill"] == 0, (k, v)
        assert v["lds"] == 0, (k, v)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_ps_and_flags_are_the_trace_backs_bits(oracle_lib, name):
    p, o, d, w = records(oracle_lib, name)
    cam = _camera(p)
    O, D = ray_sets(cam.info(), p, o, d, w)
    ps, fl, J = jr.host_jacobian(cam, O, D)
    ps0, fl0 = jr.host_trace(cam, O, D)
    assert _same_bits(ps, ps0) and np.array_equal(fl, fl0)
    traced = (fl & 1) == 1
    assert traced.sum() > 0.9 * (w > 0).sum()
    assert len(set(tc.reason(fl[~traced]).tolist())) >= (3 if int(p["lensModel"]) == RAYTRACED else 2)
    assert (J[~traced].view(np.uint32) == 0).all()          # twelve +0.0
    assert (np.abs(J[traced]).max((1, 2)) > 0).all()
    # the spectral call: at 587.5618 nm the d-line's bits, J included; with a wavelength per ray, zoic_trace_back_ray_spectral's
    ps1, fl1, J1 = jr.host_jacobian(cam, O, D, LAMBDA_D)
    assert _same_bits(ps1, ps) and np.array_equal(fl1, fl) and _same_bits(J1, J)
    cam.close()


@pytest.mark.parametrize("name", list(SPECTRAL) + ["C1"])
def test_spectral_ps_and_flags_are_the_spectral_trace_backs_bits(oracle_lib, name):
    p, o, d, w = records(oracle_lib, name)
    cam = _camera(p, name, spectral=name in SPECTRAL)
    O, D = ray_sets(cam.info(), p, o[::4], d[::4], w[::4])
    lam = bs.mixed_wavelengths(len(O))
    ps, fl, J = jr.host_jacobian(cam, O, D, lam)
    ps0, fl0 = jr.host_trace(cam, O, D, lam)
    assert _same_bits(ps, ps0) and np.array_equal(fl, fl0)
    traced = (fl & 1) == 1
    assert (J[~traced].view(np.uint32) == 0).all()
    bad = ~bs.valid(lam)
    assert bad.sum() > len(O) // 5 and (tc.reason(fl[bad]) == bs.TB_WAVELENGTH).all() and not traced[bad].any()
    assert traced[~bad].sum() > 0.5 * (~bad).sum() * (w > 0).mean()
    cam.close()


def test_cameras_that_trace_nothing():
    ray = ((0.05, 0.02, -3.0), (0.01, -0.02, -1.0))
    for cfg, over in (("C3", dict(lensModel=_capi.LENS_NONE)), ("C3", dict(focalLength=-10.0)), ("C1", dict(useDof=False))):
        cam = _camera(dict(camera_params(cfg), **over))
        for lam in (None, 550.0):
            sx, sy, f, J = cam.trace_back_ray_jacobian(*ray, wavelength=lam)
            assert (sx, sy, f) == cam.trace_back_ray(*ray, wavelength=lam) and f & 1 == 0
            assert np.array([sx, sy], np.float32).view(np.uint32).tolist() == [0, 0]
            assert J.shape == (2, 6) and J.dtype == np.float32 and (J.view(np.uint32) == 0).all()
        cam.close()


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
_ACC = {}


def accuracy(oracle_lib, name, spectral=False):
    """everything tests 4-8 share for one configuration (cached)"""
    key = (name, spectral)
    if key in _ACC:
        return _ACC[key]
    p, o, d, w = records(oracle_lib, name)
    cam = _camera(p, name, spectral)
    info = cam.info()
    s = jr.scales(info, p)
    live_all = np.flatnonzero(w > 0)
    stride = 16
    while stride > 1 and len(live_all[::stride]) * (1.0 - LEFT_OUT_CAP) < MIN_RAYS:
        stride //= 2
    live = live_all[::stride]
    d = d[live]
    o = (o[live].astype(np.float64) + s[0] * d.astype(np.float64)).astype(np.float32)   # one scale out along the ray: the same line
    if spectral:
        T = bs.SpectralTraceBack(info, p, cam.dispersion())
        lam = np.linspace(400.0, 700.0, 16).astype(np.float32)[np.arange(len(o)) % 16]   # spread over the rays

        def trace(O, D):
            return T.trace_at(O, D, np.tile(lam, len(O) // len(lam)))
    else:
        T, lam, trace = TraceBack(info, p), None, None
        trace = T.trace
    A = jr.measure(cam, trace, T.edge, o, d, lam, s, tag=name + (" spectral" if spectral else ""))
    _ACC[key] = dict(A, p=p, T=T, stride=stride)
    return _ACC[key]


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_reference_is_sound(oracle_lib, name):
    """f64 central differences carry an h^2 term: the steps 1e-5 s and 1e-6 s agree to 1e-7 on the kept rays"""
    A = accuracy(oracle_lib, name)
    kept = _best(A)["kept"]
    e = jr.rel_error(A["Jref5"][kept], A["Jref"][kept], A["s"])
    print("%s: Jref(1e-5) against Jref(1e-6): max %.3g" % (name, e.max()))
    assert e.max() <= 1e-7, e.max()


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_accuracy_against_the_finite_difference_yardstick(oracle_lib, name):
    _check_accuracy(accuracy(oracle_lib, name), name)


@pytest.mark.parametrize("name", list(SPECTRAL))
def test_spectral_accuracy_against_the_finite_difference_yardstick(oracle_lib, name):
    A = accuracy(oracle_lib, name, spectral=True)
    kept = _best(A)["kept"]
    e = jr.rel_error(A["Jref5"][kept], A["Jref"][kept], A["s"])
    assert e.max() <= 1e-7, e.max()
    _check_accuracy(A, name + " spectral")


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_null_vectors(oracle_lib, name):
    """J_o . dir = 0 and J_d . dir = 0, to the p99 error of the accuracy test (the reference satisfies both exactly)"""
    A = accuracy(oracle_lib, name)
    best = _best(A)
    kept = best["kept"]
    J, d = A["J"][kept].astype(np.float64), A["d"][kept].astype(np.float64)
    scale = np.sqrt(((J * A["s"][None, None, :]) ** 2).sum((1, 2)))
    no = np.linalg.norm(np.einsum("nij,nj->ni", J[:, :, :3], d), axis=1) / scale
    nd = np.linalg.norm(np.einsum("nij,nj->ni", J[:, :, 3:], d), axis=1) / scale
    print("%s: |J_o d| max %.3g, |J_d d| max %.3g, p99 error %.3g" % (name, no.max(), nd.max(), best["j_p99"]))
    assert no.max() <= best["j_p99"] and nd.max() <= best["j_p99"], (no.max(), nd.max(), best["j_p99"])


def _thin_closed_form(info, p, o, d):
    """f64 closed form from the f32 inputs and the f32 table entries: (J (m,2,6), tau I)"""
    fd = abs(float(np.float32(p["focalDistance"])))
    I = float(np.float32(1.0) / np.float32(np.float32(fd) * np.float32(info["tan_fov"])))
    o, d = o.astype(np.float64), d.astype(np.float64)
    tau = -(o[:, 2] + fd) / d[:, 2]
    J = np.zeros((len(o), 2, 6))
    for r in (0, 1):
        J[:, r, r] = I
        J[:, r, 2] = -(d[:, r] / d[:, 2]) * I
        J[:, r, 3 + r] = tau * I
        J[:, r, 5] = (o[:, 2] + fd) * d[:, r] / d[:, 2] ** 2 * I
    return J, tau * I


@pytest.mark.parametrize("name", list(tc.THIN))
def test_thin_lens_closed_form(oracle_lib, name):
    """every entry within 32 ulp of its row's largest entry: each is a handful of correctly rounded f32 operations"""
    p, o, d, w = records(oracle_lib, name)
    cam = _camera(p)
    live = w > 0
    rng = np.random.default_rng(2)
    out = rng.uniform(0.0, 50.0, live.sum())[:, None]   # the start point anywhere on the line, and dir at any length
    O = (o[live].astype(np.float64) + out * d[live].astype(np.float64)).astype(np.float32)
    D = (d[live].astype(np.float64) * 10.0 ** rng.uniform(-2, 2, live.sum())[:, None]).astype(np.float32)
    ps, fl, J = jr.host_jacobian(cam, O, D)
    traced = (fl & 1) == 1
    assert traced.sum() > 0.9 * live.sum()
    want, _ = _thin_closed_form(cam.info(), p, O[traced], D[traced])
    got = J[traced].astype(np.float64)
    ulp = np.spacing(np.abs(got).max(2).astype(np.float32)).astype(np.float64)[:, :, None]
    worst = (np.abs(got - want) / ulp).max()
    print("%s: %d rays, worst entry %.2f ulp of its row's largest" % (name, traced.sum(), worst))
    assert worst <= 32.0, worst
    cam.close()


def _basis(u, turn):
    """a right-handed orthonormal basis (e1, e2) of the plane across u (e1 x e2 = u), turned by `turn` about u"""
    a = np.where(np.abs(u[:, :1]) < 0.6, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    e1 = np.cross(a, u)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(u, e1)
    c, s = np.cos(turn), np.sin(turn)
    return c * e1 + s * e2, -s * e1 + c * e2


@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4"])
def test_solid_angle_measure(oracle_lib, name):
    A = accuracy(oracle_lib, name)
    kept = _best(A)["kept"]
    J, d = A["J"][kept], A["d"][kept].astype(np.float64) * 3.0   # (a direction of length 3: |d| enters)
    Jd = J.copy()
    Jd[:, :, 3:] /= 3.0                                            # J_d of the same ray given with dir 3 times as long
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    m0 = solid_angle_measure(Jd, d)
    assert m0.shape == (kept.sum(),)
    for turn in (0.0, 1.1):
        e1, e2 = _basis(u, turn)
        assert np.allclose(np.cross(e1, e2), u, atol=1e-12)
        m = solid_angle_measure(Jd, d, basis=(e1, e2))
        assert np.allclose(m, m0, rtol=1e-9, atol=0.0), np.abs(m / m0 - 1).max()
    assert np.allclose(solid_angle_measure(J, d / 3.0), m0, rtol=1e-6)   # the measure belongs to the line, not to dir's length
    import torch
    mt = solid_angle_measure(torch.from_numpy(Jd), torch.from_numpy(d.astype(np.float32)))
    assert tuple(mt.shape) == m0.shape and np.allclose(mt.numpy(), m0, rtol=1e-4)
    if name == "C1":   # the closed form's determinant: (tau I)^2 |d|^3 / d.z
        o, dd = A["o"][kept], A["d"][kept]
        _, tauI = _thin_closed_form(A["cam"].info(), A["p"], o, dd)
        dd = dd.astype(np.float64)
        want = tauI ** 2 * np.linalg.norm(dd, axis=1) ** 3 / dd[:, 2]
        got = solid_angle_measure(J, dd)
        assert np.allclose(got, want, rtol=1e-5), np.abs(got / want - 1).max()
    else:
        assert (np.sign(m0) == np.sign(m0[0])).all() and m0[0] != 0.0
    print("%s: dPs/domega %.4g ... %.4g" % (name, m0.min(), m0.max()))


def test_errors():
    from zoic_amd.camera import ZoicError
    lib = _capi.load()
    o, d = _capi.Vec3(0.05, 0.02, -3.0), _capi.Vec3(0.0, 0.0, -1.0)
    ps, J, f = (ctypes.c_float * 2)(), (ctypes.c_float * 12)(), ctypes.c_uint32()
    B = ctypes.byref
    assert lib.zoic_trace_back_ray_jacobian(None, B(o), B(d), ps, B(f), J) == 1
    assert lib.zoic_trace_back_jacobian_device(None, 4, None, None, None, None, None) == 1
    fresh = ZoicCamera(device=-1)
    with pytest.raises(ZoicError) as e:
        fresh.trace_back_ray_jacobian((0.05, 0.02, -3.0), (0.0, 0.0, -1.0))
    assert e.value.status_name == "ZOIC_ERR_NOT_UPDATED"
    fresh.close()
    cam = _camera(camera_params("C2"))
    for call, extra in ((lib.zoic_trace_back_ray_jacobian, ()), (lib.zoic_trace_back_ray_jacobian_spectral, (ctypes.c_float(550.0),))):
        assert call(cam._h, None, B(d), *extra, ps, None, J) == 1
        assert call(cam._h, B(o), None, *extra, ps, None, J) == 1
        assert call(cam._h, B(o), B(d), *extra, None, None, J) == 1
        assert call(cam._h, B(o), B(d), *extra, ps, None, None) == 1
        assert call(cam._h, B(o), B(d), *extra, ps, None, J) == 0   # flags may be NULL
    for lam in (None, np.full(4, 550.0, np.float32)):
        with pytest.raises(ZoicError) as e:   # a tables-only camera has no device
            cam.trace_back_jacobian(np.zeros((4, 8), np.float32), wavelengths=lam)
        assert e.value.status_name == "ZOIC_ERR_NO_DEVICE"
    cam.close()

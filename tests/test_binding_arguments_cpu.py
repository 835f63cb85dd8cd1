"""The Python binding's argument rules without a GPU, on a tables-only camera (device=-1): what zoic_amd/camera.py refuses before it
calls the library, what it hands to the library when it does not, and the bits of the host single-item calls.

The numpy halves of the batch calls refuse a wrong item width or rank and a caller's out / flags / jacobian with ValueError, a torch
tensor next to numpy items with TypeError, and pass well-formed input on: the library then reports ZOIC_ERR_NO_DEVICE from the same
entry point with the same number of arguments as ever (recorded by a proxy in front of the loaded library).  The torch halves refuse a
host tensor with ValueError before anything of torch.cuda is touched.  The host single-item calls give, with and without a wavelength,
the bits of the suite's host twins: the raw C-ABI drivers of traceback_cases.py and traceback_jacobian_ref.py, and the host builds of
csrc/pupil_bounds.hpp and csrc/splat.hpp."""
import functools

import numpy as np
import pytest
import torch

from zoic_amd import ZoicCamera, _capi
from zoic_amd.camera import ZoicError

import backward_spectral_ref as bs
import pupil_cases as pc
import pupil_driver
import splat_driver
import splat_ref
import traceback_cases as tc
import traceback_jacobian_ref as tj

F32 = np.float32
N, K, M = 5, 2, 1
NO_DEVICE = _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")
LAMBDA = 450.0


@functools.lru_cache(maxsize=None)
def _camera():
    """the double Gauss with its dispersion table, tables-only"""
    p = pc.params_of("C3")
    cam = tc.update(ZoicCamera(device=-1), p)
    bs.set_dispersion(cam, pc.CAMERAS["C3"][0])
    return cam, p


class _Recorder:
    """stands in front of the loaded library: notes (entry point, number of arguments) of every call and passes it on"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, len(args)))
            return fn(*args)
        return call


def _items(width):
    return np.linspace(-0.5, 0.5, N * width, dtype=F32).reshape(N, width)


S, P, R = _items(4), _items(3), _items(8)
W, WK = np.full(N, LAMBDA, F32), np.full((N, K), LAMBDA, F32)
B = np.zeros(N, _capi.PUPIL_BOUNDS_DTYPE)
U = np.zeros((N, M, 2), F32)
RECORDS = np.ascontiguousarray(R).view(_capi.RAY_DTYPE).reshape(-1)

# name -> (call(cam, items, wavelengths, **kw), good items, wavelengths (None: the call has a d-line form too), the keywords for
#          caller-given results, (d-line probe, spectral probe): the entry point and the number of arguments of each)
NUMPY_CALLS = {
    "create_rays(wavelengths=)": (lambda c, x, w, **kw: c.create_rays(x, wavelengths=w, **kw), S, W, ("out",),
                                  (None, ("zoic_create_rays_spectral_device", 8))),
    "create_rays_hero": (lambda c, x, w, **kw: c.create_rays_hero(x, w, **kw), S, WK, ("out",), (None, ("zoic_create_rays_hero_device", 9))),
    "project_points": (lambda c, x, w, **kw: c.project_points(x, wavelengths=w, **kw), P, None, ("out", "flags"),
                       (("zoic_project_points_device", 6), ("zoic_project_points_spectral_device", 7))),
    "trace_back": (lambda c, x, w, **kw: c.trace_back(x, wavelengths=w, **kw), R, None, ("out", "flags"),
                   (("zoic_trace_back_rays_device", 6), ("zoic_trace_back_rays_spectral_device", 7))),
    "trace_back_jacobian": (lambda c, x, w, **kw: c.trace_back_jacobian(x, wavelengths=w, **kw), R, None, ("out", "flags", "jacobian"),
                            (("zoic_trace_back_jacobian_device", 7), ("zoic_trace_back_jacobian_spectral_device", 8))),
    "pupil_bounds": (lambda c, x, w, **kw: c.pupil_bounds(x, wavelengths=w, **kw), P, None, ("out",),
                     (("zoic_pupil_bounds_device", 7), ("zoic_pupil_bounds_device", 7))),
    "splat_points": (lambda c, x, w, **kw: c.splat_points(x, B, U, wavelengths=w, **kw), P, None, ("out",),
                     (("zoic_splat_points_device", 8), ("zoic_splat_points_device", 8))),
}


def _refusals():
    """(id, call name, items, wavelengths, keywords, exception)"""
    rows = []
    for name, (_, x, w, results, _) in NUMPY_CALLS.items():
        wide = np.concatenate([x, x[:, :1]], 1)
        rows.append((name + "-width", name, wide, w, {}, ValueError))
        rows.append((name + "-rank", name, x.reshape(-1), w, {}, ValueError))
        rows.append((name + "-rank3", name, x.reshape(N, 1, -1), w, {}, ValueError))
        for kw in results:
            rows.append((name + "-" + kw, name, x, w, {kw: np.zeros((N, 2), F32)}, ValueError))
        tw = torch.full((N,), LAMBDA) if w is None or w.ndim == 1 else torch.full((N, K), LAMBDA)
        rows.append((name + "-torch-wavelengths", name, x, tw, {}, TypeError))
    for name in ("create_rays(wavelengths=)", "create_rays_hero"):
        _, x, w, _, _ = NUMPY_CALLS[name]
        rows.append((name + "-torch-rng_states", name, x, w, dict(rng_states=torch.zeros((N, 4), dtype=torch.int32)), TypeError))
    rows.append(("create_rays_hero-wavelength-rank", "create_rays_hero", S, W, {}, ValueError))
    rows.append(("create_rays_hero-wavelength-rows", "create_rays_hero", S, WK[:-1], {}, ValueError))
    return rows


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_numpy_half_refuses(case):
    _, name, x, w, kw, exc = case
    cam, _ = _camera()
    rec = _Recorder(cam._lib)
    cam._lib = rec
    try:
        with pytest.raises(exc):
            NUMPY_CALLS[name][0](cam, x, w, **kw)
    finally:
        cam._lib = rec._lib
    assert rec.calls == []   # refused in Python: the library has not been asked


def test_splat_points_refuses_torch_bounds_and_u_next_to_numpy_points():
    cam, _ = _camera()
    with pytest.raises(TypeError):
        cam.splat_points(P, torch.zeros((N, 12)), U)
    with pytest.raises(TypeError):
        cam.splat_points(P, B, torch.zeros((N, M, 2)))


def _well_formed():
    rows = []
    for name, (_, x, w, _, (dline, spectral)) in NUMPY_CALLS.items():
        if dline is not None:
            rows.append((name + "-dline", name, x, None, dline))
        rows.append((name + "-spectral", name, x, W if w is None else w, spectral))
    rows.append(("trace_back-records", "trace_back", RECORDS, None, NUMPY_CALLS["trace_back"][4][0]))
    rows.append(("trace_back-dict", "trace_back", dict(rays=RECORDS), W, NUMPY_CALLS["trace_back"][4][1]))
    rows.append(("trace_back_jacobian-dict", "trace_back_jacobian", dict(rays=RECORDS), None, NUMPY_CALLS["trace_back_jacobian"][4][0]))
    rows.append(("project_points-f64-lists", "project_points", P.astype(np.float64).tolist(), None, NUMPY_CALLS["project_points"][4][0]))
    return rows


@pytest.mark.parametrize("case", _well_formed(), ids=lambda c: c[0])
def test_well_formed_numpy_input_reaches_the_library(case):
    """a tables-only camera: the probing call is the only call, and it is the entry point and the argument count it always was"""
    _, name, x, w, probe = case
    cam, _ = _camera()
    rec = _Recorder(cam._lib)
    cam._lib = rec
    try:
        with pytest.raises(ZoicError) as e:
            NUMPY_CALLS[name][0](cam, x, w)
    finally:
        cam._lib = rec._lib
    assert e.value.status == NO_DEVICE
    assert [c for c in rec.calls if c[0] != "zoic_last_error_string"] == [probe]


def test_splat_points_takes_the_bounds_as_records_or_floats():
    cam, _ = _camera()
    for bounds in (B, np.zeros((N, 12), F32)):
        with pytest.raises(ZoicError) as e:
            cam.splat_points(P, bounds, U, wavelengths=W)
        assert e.value.status == NO_DEVICE


# ---- the torch halves, given host tensors ----------------------------------------------------------------------------------------
TS, TP, TR = torch.from_numpy(S), torch.from_numpy(P), torch.from_numpy(R)
TW, TWK = torch.from_numpy(W), torch.from_numpy(WK)
TB, TU = torch.zeros((N, 12)), torch.from_numpy(U)
PAIRS = np.array([[1, 0]])
HOST_TENSOR_CALLS = {
    "create_rays": lambda c: c.create_rays(TS),
    "create_rays(wavelengths=)": lambda c: c.create_rays(TS, wavelengths=TW),
    "create_rays_hero": lambda c: c.create_rays_hero(TS, TWK),
    "project_points": lambda c: c.project_points(TP),
    "project_points(wavelengths=)": lambda c: c.project_points(TP, wavelengths=TW),
    "trace_back": lambda c: c.trace_back(TR),
    "trace_back-dict": lambda c: c.trace_back(dict(rays=TR), wavelengths=TW),
    "trace_back_jacobian": lambda c: c.trace_back_jacobian(TR),
    "pupil_bounds": lambda c: c.pupil_bounds(TP),
    "pupil_bounds(wavelengths=)": lambda c: c.pupil_bounds(TP, wavelengths=TW),
    "splat_points": lambda c: c.splat_points(TP, TB, TU),
    "ray_differentials": lambda c: c.ray_differentials(TS, TR),
    "ray_differentials(wavelengths=)": lambda c: c.ray_differentials(TS, dict(rays=TR), wavelengths=TW, chromatic=True),
    "transmittance": lambda c: c.transmittance(TS, TR),
    "transmittance-hero": lambda c: c.transmittance(TS, TR.reshape(N, 1, 8).repeat(1, K, 1), wavelengths=TWK),
    "create_ghost_rays": lambda c: c.create_ghost_rays(TS, TR, PAIRS),
}


@pytest.fixture
def no_torch_cuda(monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("torch.cuda was touched")
    for name in ("current_stream", "synchronize", "current_device", "set_device"):
        monkeypatch.setattr(torch.cuda, name, touched)


def _refused_without_the_library(cam, call):
    rec = _Recorder(cam._lib)
    cam._lib = rec
    try:
        with pytest.raises(ValueError):
            call(cam)
    finally:
        cam._lib = rec._lib
    assert rec.calls == []


@pytest.mark.parametrize("name", sorted(HOST_TENSOR_CALLS))
def test_torch_half_refuses_a_host_tensor(name, no_torch_cuda):
    _refused_without_the_library(_camera()[0], HOST_TENSOR_CALLS[name])


def test_resident_call_refuses_a_host_tensor(no_torch_cuda):
    """create_rays_resident used to check neither is_cuda nor the device index (tests/test_binding_arguments_gpu.py has the device
    side of this rule)"""
    cam, _ = _camera()
    _refused_without_the_library(cam, lambda c: c.create_rays_resident(TS))
    _refused_without_the_library(cam, lambda c: c.create_rays_resident(TS, out=torch.zeros((N, 8))))


def test_ray_differentials_chromatic_needs_wavelengths():
    with pytest.raises(ValueError):
        _camera()[0].ray_differentials(TS, TR, chromatic=True)


# ---- the host single-item calls --------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _rays(cam, p):
    """the ten scene points of pupil_cases and a ray from each towards the front element"""
    pts = pc.points(p)
    aim = np.array([0.1, -0.05, cam.pupil_square()[0]], F32)
    return pts, pts, (pts - aim).astype(F32)


@pytest.mark.parametrize("lam", (None, LAMBDA), ids=("dline", "spectral"))
def test_single_item_calls_give_the_host_twins_bits(lam):
    cam, p = _camera()
    pts, o, d = _rays(cam, p)
    lams = None if lam is None else np.full(len(pts), lam, F32)
    finite = np.isfinite(pts).all(1)
    # project_point and trace_back_ray against the raw C-ABI drivers
    ps, fl = tc.lib_project(cam, pts, lams)
    got = [cam.project_point(q, lam) for q in pts]
    assert np.array_equal(_bits([g[:2] for g in got]), _bits(ps)) and [g[2] for g in got] == fl.tolist()
    assert (fl[finite] & 1).any()
    ps, fl = tc.lib_trace(cam, o, d, lams)
    got = [cam.trace_back_ray(o[i], d[i], lam) for i in range(len(o))]
    assert np.array_equal(_bits([g[:2] for g in got]), _bits(ps)) and [g[2] for g in got] == fl.tolist()
    assert (fl & 1).any()
    # trace_back_ray_jacobian
    ps, fl, J = tj.host_jacobian(cam, o, d, lams)
    got = [cam.trace_back_ray_jacobian(o[i], d[i], lam) for i in range(len(o))]
    assert np.array_equal(_bits([g[:2] for g in got]), _bits(ps)) and [g[2] for g in got] == fl.tolist()
    assert np.array_equal(_bits(np.stack([g[3] for g in got])), _bits(J)) and J[(fl & 1) == 1].any()
    assert all(type(g[0]) is float and type(g[2]) is int and g[3].shape == (2, 6) and g[3].dtype == F32 for g in got)
    # pupil_bounds_point against the host build of csrc/pupil_bounds.hpp, with and without a film window
    disp = None if lam is None else cam.dispersion()
    for window in (None, pc.WINDOW):
        ref = pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, 16, window, lams, disp)
        for i, q in enumerate(pts):
            r = cam.pupil_bounds_point(q, 16, window, lam)
            assert sorted(r) == ["aim", "count", "flags", "lattice", "screen"]
            assert np.array_equal(_bits(r["aim"]), _bits(ref["aim"][i])) and np.array_equal(_bits(r["screen"]), _bits(ref["screen"][i]))
            assert (r["count"], r["lattice"], r["flags"]) == (ref["count"][i], ref["lattice"][i], ref["flags"][i])
    assert (ref["count"] > 0).any()
    # splat_point against the host build of csrc/splat.hpp
    ref_b = pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, 16, None, lams, disp)
    u = np.random.default_rng(4).random((len(pts), 3, 2)).astype(F32)
    ref = splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, ref_b, u, lams, disp)
    got = np.stack([cam.splat_point(pts[i], ref_b[i:i + 1], u[i], lam) for i in range(len(pts))])
    assert got.dtype == np.dtype(_capi.SPLAT_DTYPE) and splat_ref.same_records(got, ref), splat_ref.differing(got, ref)
    assert (ref["flags"] & 1).any()


def test_pupil_window_must_have_four_numbers():
    cam, p = _camera()
    with pytest.raises(ValueError):
        cam.pupil_bounds_point(pc.points(p)[0], 16, (0.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        cam.pupil_bounds(P, window=(0.0, 0.0, 1.0))


def test_table_getters_equal_the_library():
    """dispersion(), coatings() and ghost_pairs(): the arrays the C-ABI fills, asked for directly"""
    cam, p = _camera()
    lib, h = _capi.load(), cam._h
    cam.set_coatings(np.linspace(1.3, 1.4, 11, dtype=F32), 550.0)
    try:
        count = cam.info()["lensCount"]
        n = lib.zoic_camera_get_dispersion(h, 0, None, None, None)
        assert n == count
        raw = [np.zeros(n, F32) for _ in range(3)]
        assert lib.zoic_camera_get_dispersion(h, n, *[a.ctypes.data for a in raw]) == n
        got = cam.dispersion()
        assert sorted(got) == ["abbe", "cauchy_b", "ior_d"]
        for k, a in zip(("ior_d", "abbe", "cauchy_b"), raw):
            assert got[k].dtype == F32 and np.array_equal(_bits(got[k]), _bits(a)), k
        assert got["cauchy_b"].any()
        raw = [np.zeros(n, F32) for _ in range(2)]
        assert lib.zoic_camera_get_coatings(h, 0, None, None) == n == lib.zoic_camera_get_coatings(h, n, *[a.ctypes.data for a in raw])
        got = cam.coatings()
        assert sorted(got) == ["index", "lambda0_nm"]
        for k, a in zip(("index", "lambda0_nm"), raw):
            assert got[k].dtype == F32 and np.array_equal(_bits(got[k]), _bits(a)), k
        assert got["index"].any() and (got["lambda0_nm"][got["index"] != 0] == 550.0).all()
        m = lib.zoic_camera_get_ghost_pairs(h, 0, None)
        packed = np.zeros(m, np.uint32)
        assert lib.zoic_camera_get_ghost_pairs(h, m, packed.ctypes.data) == m > 0
        got = cam.ghost_pairs()
        assert got.dtype == np.int32 and got.shape == (m, 2)
        assert np.array_equal(got[:, 0], packed & 255) and np.array_equal(got[:, 1], (packed >> 8) & 255) and (got[:, 0] > got[:, 1]).all()
    finally:
        cam.set_coatings(None, None)


def test_table_getters_report_a_camera_without_tables():
    """a camera that was never updated: the size query fails and the library's own status and detail surface"""
    fresh = ZoicCamera(device=-1)
    lib = _capi.load()
    for name, nargs in (("dispersion", 3), ("coatings", 2), ("ghost_pairs", 1)):
        n = getattr(lib, "zoic_camera_get_" + name)(fresh._h, 0, *[None] * nargs)
        if n < 0:
            with pytest.raises(ZoicError) as e:
                getattr(fresh, name)()
            assert e.value.status == 1 and (lib.zoic_last_error_string() or b"").decode() in str(e.value)
        else:
            got = getattr(fresh, name)()
            assert len(got) == n or all(len(v) == n for v in got.values())
    fresh.close()

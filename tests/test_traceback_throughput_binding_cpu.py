"""The binding's argument rules for the four trace-back transmittance methods without a GPU, in the manner of
tests/test_binding_arguments_cpu.py: the numpy halves refuse a wrong width or rank
and a caller's result buffers with ValueError and a torch tensor next to numpy items with TypeError, before the library is asked;
well-formed numpy input -- records, the dict of a create_rays call, bounds as records or floats -- reaches the one probing call; the
torch halves refuse a host tensor before torch.cuda is touched; and the host single-item methods give the raw C-ABI calls' bits."""
import functools

import numpy as np
import pytest
import torch

from zoic_amd import ZoicCamera, _capi
from zoic_amd.camera import ZoicError

import backward_spectral_ref as bs
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr

N, M = 5, 1
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
    return np.linspace(-0.5, 0.5, N * width, dtype=np.float32).reshape(N, width)


P, R = _items(3), _items(8)
W = np.full(N, LAMBDA, np.float32)
B = np.zeros(N, _capi.PUPIL_BOUNDS_DTYPE)
U = np.zeros((N, M, 2), np.float32)
RECORDS = np.ascontiguousarray(R).view(_capi.RAY_DTYPE).reshape(-1)
TP, TR, TW = torch.from_numpy(P), torch.from_numpy(R), torch.from_numpy(W)
TB, TU = torch.zeros((N, 12)), torch.from_numpy(U)

F32 = np.float32
# name -> (call(cam, items, wavelengths, **kw), good items, the keywords for caller-given results, the probe: entry point, arguments)
NUMPY_CALLS = {
    "trace_back_transmittance": (lambda c, x, w, **kw: c.trace_back_transmittance(x, wavelengths=w, **kw), R, ("out", "screen", "flags"),
                                 ("zoic_trace_back_transmittance_device", 7)),
    "splat_transmittance": (lambda c, x, w, **kw: c.splat_transmittance(x, B, U, wavelengths=w, **kw), P, ("out",),
                            ("zoic_splat_transmittance_device", 8)),
}


def _refusals():
    rows = []
    for name, (_, x, results, _) in NUMPY_CALLS.items():
        rows.append((name + "-width", name, np.concatenate([x, x[:, :1]], 1), None, {}, ValueError))
        rows.append((name + "-rank", name, x.reshape(-1), None, {}, ValueError))
        rows.append((name + "-rank3", name, x.reshape(N, 1, -1), W, {}, ValueError))
        for kw in results:
            rows.append((name + "-" + kw, name, x, None, {kw: np.zeros((N, 2), F32)}, ValueError))
        rows.append((name + "-torch-wavelengths", name, x, torch.full((N,), LAMBDA), {}, TypeError))
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


def test_splat_transmittance_refuses_torch_bounds_and_u_next_to_numpy_points():
    cam, _ = _camera()
    with pytest.raises(TypeError):
        cam.splat_transmittance(P, torch.zeros((N, 12)), U)
    with pytest.raises(TypeError):
        cam.splat_transmittance(P, B, torch.zeros((N, M, 2)))


WELL_FORMED = [("trace_back_transmittance-dline", "trace_back_transmittance", R, None),
               ("trace_back_transmittance-spectral", "trace_back_transmittance", R, W),
               ("trace_back_transmittance-records", "trace_back_transmittance", RECORDS, None),
               ("trace_back_transmittance-dict", "trace_back_transmittance", dict(rays=RECORDS), W),
               ("trace_back_transmittance-f64-lists", "trace_back_transmittance", R.astype(np.float64).tolist(), None),
               ("splat_transmittance-dline", "splat_transmittance", P, None),
               ("splat_transmittance-spectral", "splat_transmittance", P, W)]


@pytest.mark.parametrize("case", WELL_FORMED, ids=lambda c: c[0])
def test_well_formed_numpy_input_reaches_the_library(case):
    """a tables-only camera: the probing call is the only call"""
    _, name, x, w = case
    cam, _ = _camera()
    rec = _Recorder(cam._lib)
    cam._lib = rec
    try:
        with pytest.raises(ZoicError) as e:
            NUMPY_CALLS[name][0](cam, x, w)
    finally:
        cam._lib = rec._lib
    assert e.value.status == NO_DEVICE
    assert [c for c in rec.calls if c[0] != "zoic_last_error_string"] == [NUMPY_CALLS[name][3]]


def test_splat_transmittance_takes_the_bounds_as_records_or_floats():
    cam, _ = _camera()
    for bounds in (B, np.zeros((N, 12), F32)):
        with pytest.raises(ZoicError) as e:
            cam.splat_transmittance(P, bounds, U, wavelengths=W)
        assert e.value.status == NO_DEVICE


HOST_TENSOR_CALLS = {
    "trace_back_transmittance": lambda c: c.trace_back_transmittance(TR),
    "trace_back_transmittance-dict": lambda c: c.trace_back_transmittance(dict(rays=TR), wavelengths=TW),
    "trace_back_transmittance-out": lambda c: c.trace_back_transmittance(TR, out=torch.zeros(N), screen=torch.zeros((N, 2)),
                                                                         flags=torch.zeros(N, dtype=torch.int32)),
    "splat_transmittance": lambda c: c.splat_transmittance(TP, TB, TU),
    "splat_transmittance(wavelengths=)": lambda c: c.splat_transmittance(TP, TB, TU, TW, out=torch.zeros((N, M))),
}


@pytest.fixture
def no_torch_cuda(monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("torch.cuda was touched")
    for name in ("current_stream", "synchronize", "current_device", "set_device"):
        monkeypatch.setattr(torch.cuda, name, touched)


@pytest.mark.parametrize("name", sorted(HOST_TENSOR_CALLS))
def test_torch_half_refuses_a_host_tensor(name, no_torch_cuda):
    cam = _camera()[0]
    rec = _Recorder(cam._lib)
    cam._lib = rec
    try:
        with pytest.raises(ValueError):
            HOST_TENSOR_CALLS[name](cam)
    finally:
        cam._lib = rec._lib
    assert rec.calls == []


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("lam", (None, LAMBDA), ids=("dline", "spectral"))
def test_single_item_methods_give_the_library_calls_bits(lam):
    cam, p = _camera()
    pts = pc.points(p)      # the ten scene points of pupil_cases and a ray from each towards the front element
    o, d = pts, (pts - np.array([0.1, -0.05, cam.pupil_square()[0]], F32)).astype(F32)
    ps, fl, T = tr.lib_throughput(cam, o, d, None if lam is None else np.full(len(o), lam, F32))
    got = [cam.trace_back_ray_transmittance(o[i], d[i], lam) for i in range(len(o))]
    assert np.array_equal(_bits([g[:2] for g in got]), _bits(ps)) and [g[2] for g in got] == fl.tolist()
    assert np.array_equal(_bits([g[3] for g in got]), _bits(T)) and (T > 0).any()
    assert all(type(g[0]) is float and type(g[2]) is int and type(g[3]) is float for g in got)
    assert [g[:3] for g in got] == [cam.trace_back_ray(o[i], d[i], lam) for i in range(len(o))]
    # splat_point_transmittance: the bounds as the dict of pupil_bounds_point, as one record and as its twelve floats
    u = np.random.default_rng(4).random((len(pts), 3, 2)).astype(F32)
    seen = 0
    for i, q in enumerate(pts):
        b = cam.pupil_bounds_point(q, 16, None, lam)
        rec = np.zeros(1, _capi.PUPIL_BOUNDS_DTYPE)
        rec[0] = (b["aim"], b["screen"], b["count"], b["lattice"], b["flags"], 0)
        t = cam.splat_point_transmittance(q, b, u[i], lam)
        assert t.dtype == F32 and t.shape == (3,)
        for other in (rec, rec.view(F32).reshape(1, 12)):
            assert np.array_equal(_bits(cam.splat_point_transmittance(q, other, u[i], lam)), _bits(t))
        s = cam.splat_point(q, b, u[i], lam)
        assert np.array_equal(t > 0, (s["flags"] & 1) == 1)
        seen += int((t > 0).sum())
    assert seen >= 6
    with pytest.raises(ValueError):
        cam.splat_point_transmittance(pts[0], np.zeros(2, _capi.PUPIL_BOUNDS_DTYPE), u[0])
    with pytest.raises(ValueError):
        cam.splat_point_transmittance(pts[0], b, u[0].reshape(-1))

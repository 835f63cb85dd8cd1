"""The backward paths at a wavelength per item on the MI355X (zoic_trace_back_rays_spectral_device,
zoic_project_points_spectral_device): both kernels give their host calls' bits, flags included, with valid and rejected wavelengths
interleaved inside one wave and whatever the batch size; at 587.5618 nm they give the d-line kernels' bits; the records the forward
spectral kernel writes come back, on the buffer they were written to, to the samples they were made from -- which the d-line
trace-back of the same records misses by the lens's chromatic aberration; bad pointers are refused before any launch."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import traceback_cases as tc
from reverse_ref import kolb_point_set, thin_point_set
from device_cases import bits as _bits, records as _records
from traceback_cases import lib_project, lib_trace
from traceback_ref import TraceBack

F32 = np.float32
SIZES = (1, 63, 64, 65, 524289)   # 524 289 = one grid of 2048 x 256 lanes and one item more
CONFIGS = ["C1", "C2", "C3", "C4", "C5"]


def _camera(name, device=0):
    p = tc.params_of(name)
    cam = ZoicCamera(device=device)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    if device >= 0:
        cam.set_precision(PRECISION_STRICT)
    cam.update(**p)
    return bs.set_dispersion(cam, name), p


def _tb_set(oracle_lib, cam, name):
    rec = tc.oracle_records(oracle_lib, tc.params_of(name))[1:]
    o, d = bs.trace_back_rays(tc, cam.info(), rec, name in tc.KOLB)
    return _records(o, d)


def _point_set(cam, p, name):
    info = cam.info()
    if name in tc.THIN:
        return thin_point_set(float(info["tan_fov"]), p["focalDistance"])[0]
    return kolb_point_set(info, p["sensorWidth"], p["focalDistance"])[0]


def _batches(items, lam, call, host):
    """device == host for the whole set and for every size of SIZES (the set tiled up to it)"""
    import torch
    scr, fl = call(items, lam)
    hs, hf = host
    assert np.array_equal(_bits(scr), _bits(hs)) and np.array_equal(fl.astype(np.uint32), hf)
    for n in SIZES:
        reps = -(-n // len(items))
        it = torch.from_numpy(np.tile(items, (reps, 1))[:n].copy()).to("cuda:0")
        lm = torch.from_numpy(np.tile(lam, reps)[:n].copy()).to("cuda:0")
        s, f = call(it, lm)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s.cpu().numpy()), np.tile(_bits(hs), (reps, 1))[:n]), n
        assert np.array_equal(f.cpu().numpy().astype(np.uint32), np.tile(hf, reps)[:n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_trace_back_kernel_equals_host_and_d_line_kernel_bitwise(gpu, oracle_lib, name):
    import torch
    cam, p = _camera(name)
    rays = _tb_set(oracle_lib, cam, name)
    lam = bs.mixed_wavelengths(len(rays))
    host = lib_trace(cam, rays[:, 0:3], rays[:, 3:6], lam)
    bad = ~bs.valid(lam)
    assert (tc.reason(host[1][bad]) == bs.TB_WAVELENGTH).all() and (host[1][~bad] & 1).sum() > 1000
    _batches(rays, lam, lambda r, w: cam.trace_back(r, wavelengths=w), host)
    # at the d-line: the d-line kernel's bits
    s0, f0 = cam.trace_back(rays)
    s1, f1 = cam.trace_back(rays, wavelengths=np.full(len(rays), bs.LAMBDA_D, F32))
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1)
    # d_flags = NULL: the same samples
    t = torch.from_numpy(rays[:65].copy()).to("cuda:0")
    w = torch.from_numpy(lam[:65].copy()).to("cuda:0")
    out = torch.full((65, 2), 7.0, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert _capi.load().zoic_trace_back_rays_spectral_device(cam._h, 65, t.data_ptr(), w.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(host[0][:65]))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_projection_kernel_equals_host_and_d_line_kernel_bitwise(gpu, name):
    import torch
    cam, p = _camera(name)
    pts = np.ascontiguousarray(_point_set(cam, p, name), F32)
    nan, inf = F32(np.nan), F32(np.inf)
    pts = np.concatenate([pts, np.array([[0.1, 0.2, 1.0], [nan, 0, -10], [0, inf, -10], [0, 0, -5], [-0.0, -0.0, -5], [3, 1, -1e30]], F32)])
    lam = bs.mixed_wavelengths(len(pts))
    host = lib_project(cam, pts, lam)
    bad = ~bs.valid(lam)
    assert (((host[1][bad] >> 8) & 15) == bs.PROJECT_WAVELENGTH).all() and (host[1][~bad] & 1).sum() > 1000
    _batches(pts, lam, lambda q, w: cam.project_points(q, wavelengths=w), host)
    s0, f0 = cam.project_points(pts)
    s1, f1 = cam.project_points(pts, wavelengths=np.full(len(pts), bs.LAMBDA_D, F32))
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1)
    t = torch.from_numpy(pts[:65].copy()).to("cuda:0")
    w = torch.from_numpy(lam[:65].copy()).to("cuda:0")
    out = torch.full((65, 2), 7.0, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert _capi.load().zoic_project_points_spectral_device(cam._h, 65, t.data_ptr(), w.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(host[0][:65]))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C2", "C5", "C3"])
def test_round_trip_with_the_forward_spectral_kernel(gpu, name):
    """STRICT camera, wavelengths uniform in [400, 700] nm per ray: create_rays(samples, wavelengths) then trace_back(rays, wavelengths)
    on the same stream and buffer.  Every record of weight > 0 outside the edge set comes back, within 2 x the d-line round trip's
    maximum, measured here with the existing calls on the same samples.  The edge set is TraceBack.edge's (1e-2 at the stop, 1e-4
    elsewhere) on the f64 restatement of the records at their wavelengths rounded to whole nanometres (the restatement runs one pass
    per distinct wavelength; half a nanometre moves a clearance by ~1e-6).  Control: the same spectral records through the d-line
    trace_back miss, in the median, by more than the spectral round trip's maximum
    (test_backward_spectral_cpu.py::test_d_line_trace_back_of_coloured_rays_misses_by_more_than_the_round_trip_bound)."""
    import torch
    cam, p = _camera(name)
    host, _ = _camera(name, device=-1)
    T = bs.SpectralTraceBack(host.info(), p, host.dispersion())
    n = tc.N
    s = synthetic_samples(n, tc.W, tc.H, tc.SPP)
    smp = torch.from_numpy(s).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(n).view(np.int32)).to("cuda:0")
    lam_h = np.random.default_rng(23).uniform(400.0, 700.0, n).astype(F32)
    lam = torch.from_numpy(lam_h).to("cuda:0")
    # the d-line round trip of the existing calls on the same samples: the yardstick
    fwd0 = cam.create_rays(smp, rng_states=st)
    scr0, fl0 = cam.trace_back(fwd0)
    torch.cuda.synchronize()
    rec0 = fwd0["rays"].cpu().numpy()
    live0 = rec0[:, 6] > 0
    ref0 = T.trace(rec0[live0, 0:3], rec0[live0, 3:6])
    keep0 = ~T.edge(ref0) & ((fl0.cpu().numpy()[live0] & 1) == 1)
    d_max = float(np.abs(scr0.cpu().numpy()[live0].astype(np.float64) - s[live0, :2]).max(1)[keep0].max())
    # the spectral round trip, in place
    before = cam.counters()
    fwd = cam.create_rays(smp, wavelengths=lam, rng_states=st)
    after = cam.counters()
    scr, fl = cam.trace_back(fwd, wavelengths=lam)
    ctl, cfl = cam.trace_back(fwd)
    torch.cuda.synchronize()
    assert cam.counters() == after and after != before
    rec = fwd["rays"].cpu().numpy()
    scr, fl = scr.cpu().numpy(), fl.cpu().numpy().astype(np.uint32)
    live = rec[:, 6] > 0
    ref = T.trace_at(rec[live, 0:3], rec[live, 3:6], np.round(lam_h[live]))
    edge = T.edge(ref)
    print("%s: live %d, edge share %.2f %%" % (name, live.sum(), 100 * edge.mean()))
    assert live.sum() >= 8192 and edge.mean() <= 0.02, edge.mean()
    ok = (fl[live] & 1) == 1
    assert ok[~edge].all(), ((~ok & ~edge).sum(), np.unique(tc.reason(fl[live][~ok & ~edge])))
    rt = np.abs(scr[live].astype(np.float64) - s[live, :2]).max(1)[~edge]
    c_ok = ~edge & ((cfl.cpu().numpy()[live] & 1) == 1)
    control = np.abs(ctl.cpu().numpy()[live].astype(np.float64) - s[live, :2]).max(1)[c_ok]
    print("%s spectral round trip: max %.3g = %.2f x the d-line round trip's max (%.3g); control (d-line trace-back of the spectral records): "
          "median %.3g" % (name, rt.max(), rt.max() / d_max, d_max, np.median(control)))
    assert rt.max() <= 2.0 * d_max, (rt.max(), d_max)
    assert np.median(control) > rt.max(), (np.median(control), rt.max())
    cam.close()
    host.close()


@pytest.mark.gpu
def test_error_paths(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C2")
    n = 4096
    rays = cam.create_rays(torch.from_numpy(synthetic_samples(n, 64, 64, 1)).to("cuda:0"))["rays"]
    pts = (rays[:, 0:3] + 50.0 * rays[:, 3:6]).contiguous()
    lam = torch.full((n,), 500.0, dtype=torch.float32, device="cuda:0")
    out = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
    flags = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    host = np.zeros((n, 8), F32)
    fresh = ZoicCamera(device=0)
    tables = ZoicCamera(device=-1)
    tables.update(**p)
    for call, items, step in ((lib.zoic_trace_back_rays_spectral_device, rays, 8), (lib.zoic_project_points_spectral_device, pts, 2)):
        assert call(cam._h, n, items.data_ptr(), lam.data_ptr(), out.data_ptr(), flags.data_ptr(), st) == 0
        assert call(cam._h, n, None, lam.data_ptr(), out.data_ptr(), None, st) == 1
        assert call(cam._h, n, items.data_ptr(), None, out.data_ptr(), None, st) == 1
        assert call(cam._h, n, items.data_ptr(), lam.data_ptr(), None, None, st) == 1
        assert call(cam._h, n, host.ctypes.data, lam.data_ptr(), out.data_ptr(), None, st) == 1          # not device memory
        assert call(cam._h, n, items.data_ptr(), host.ctypes.data, out.data_ptr(), None, st) == 1
        assert call(cam._h, n - 1, items.data_ptr() + step, lam.data_ptr(), out.data_ptr(), None, st) == 1   # misaligned items
        assert call(cam._h, n - 1, items.data_ptr(), lam.data_ptr() + 2, out.data_ptr(), None, st) == 1      # misaligned wavelengths
        assert call(cam._h, n - 1, items.data_ptr(), lam.data_ptr(), out.data_ptr() + 4, None, st) == 1      # misaligned screen
        assert call(cam._h, n - 1, items.data_ptr(), lam.data_ptr(), out.data_ptr(), flags.data_ptr() + 2, st) == 1
        assert call(cam._h, 0, None, None, None, None, st) == 0                                              # n = 0: no-op
        assert call(fresh._h, n, items.data_ptr(), lam.data_ptr(), out.data_ptr(), None, st) == 9            # NOT_UPDATED
        assert call(tables._h, n, items.data_ptr(), lam.data_ptr(), out.data_ptr(), None, st) == _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        cam.trace_back(rays, wavelengths=lam[:-1])
    with pytest.raises(ValueError):
        cam.project_points(pts, wavelengths=lam.double())
    with pytest.raises(TypeError):
        cam.trace_back(rays, wavelengths=np.full(n, 500.0, F32))
    fresh.close()
    tables.close()
    cam.close()

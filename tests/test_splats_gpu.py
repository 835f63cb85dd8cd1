"""Lens splats on the MI355X (zoic_splat_points_device and its spectral form): the kernels -- one splat per lane, a grid-stride walk
over the n m splats -- give the host twin's records bit for bit, all 32 bytes, at every batch shape that takes another path through
the mapping; the bounds are those zoic_pupil_bounds_device wrote on the same stream, read in place; the call touches no counter and
no retry stream; bad arguments are refused before any launch; after an update or a new dispersion the call follows the new tables.

Host twin: csrc/splat.hpp compiled with clang++ (splat_driver.py), which tests/test_splats_cpu.py holds against an independent
restatement.  Cameras and points: pupil_cases.py."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import ZoicCamera, _capi, pupil_bounds_records, splat_records
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import pupil_cases as pc
import splat_driver
import splat_ref
import traceback_cases as tc

GRID_CAP = 2048   # workgroups of 256 lanes (kPassGridCap, kPassBlock: device_pass.hpp): more than GRID_CAP x 256 splats are walked with a grid stride
# (n, m): the smallest call; a wave straddling points, m no power of two; one point per wave; more aims than a workgroup; and one
# splat more than a full grid (2^19 + 1 = 3 x 174763), so that lane 0 of workgroup 0 takes a second trip (m = 3 does not divide the
# stride: the walk's remainder step carries over)
SHAPES = ((1, 1), (3, 5), (5, 64), (2, 257))
STRIDE_SHAPE = (174763, 3)
assert STRIDE_SHAPE[0] * STRIDE_SHAPE[1] == GRID_CAP * 256 + 1
G = 16
F32 = np.float32


def _camera(name):
    p = pc.params_of(name)
    cam = tc.update(ZoicCamera(device=0), p)
    if pc.CAMERAS[name][0] in bs.DISPERSIVE:
        bs.set_dispersion(cam, pc.CAMERAS[name][0])
    return cam, p


def _u(n, m):
    u = np.random.default_rng(1000 * n + m).random((n, m, 2)).astype(F32)
    u[0, 0] = (0.5, 0.5)                               # the box's centre: traced from the point on the axis
    u[0, m - 1] = (0.0, F32(1.0) - F32(2.0 ** -24)) if m > 1 else u[0, 0]   # a corner of the box
    if m > 2:
        u[n // 2, 1] = (np.nan, 0.5)     # a NaN aim: refused by the trace
        u[n - 1, 2] = (-1.0, 2.0)        # outside the unit square: the box's edge
    return u


def _device(cam, pts, u, lam=None, stream=None):
    """the pipeline on one stream: pupil bounds, then the splats from those bounds in place; (bounds (n,), splats (n, m)) on the host"""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        P, Uu = torch.from_numpy(pts).to(dev), torch.from_numpy(u).to(dev)
        L = None if lam is None else torch.from_numpy(lam).to(dev)
        bounds = cam.pupil_bounds(P, G, None, L)
        out = cam.splat_points(P, bounds, Uu, L)
    s.synchronize()
    assert tuple(out.shape) == (len(pts), u.shape[1], 8) and out.dtype == torch.float32
    return pupil_bounds_records(bounds), splat_records(out)


def _host(cam, p, pts, bounds, u, lam=None):
    return splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, bounds, u, lam, None if lam is None else cam.dispersion())


def _rows_present(pts, lam, bounds, host):
    """the rows every shape that holds them must show: an empty box, behind the lens, non-finite, an invalid wavelength"""
    n = len(pts)
    assert (bounds["count"] > 0).any() and ((host["flags"] & 1) == 1).any()
    if n >= 10:
        assert (host["flags"][8] == splat_ref.NO_BOX).all() and pts[8, 2] > 0            # behind the lens
        assert (host["flags"][9] == splat_ref.NO_BOX).all() and np.isnan(pts[9, 0])      # non-finite
    if n >= 4 and lam is not None:
        assert lam[3] == F32(pc.BAD_LAMBDA) and (host["flags"][3] == splat_ref.NO_BOX).all()
    if host.shape[1] > 2 and bounds["count"][n // 2] > 0:
        assert host["flags"][n // 2, 1] == 5 << 8 and np.isnan(host["ax"][n // 2, 1])    # the NaN aim: NON_FINITE


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C3", "C1", "C3-f8"])
def test_kernel_equals_host_twin_bitwise(gpu, name):
    cam, p = _camera(name)
    for n, m in SHAPES + ((10, 7),):
        pts, u = pc.batch(p, n), _u(n, m)
        lam = np.resize(pc.wavelengths(10), n).astype(F32)
        for w in (None, lam):
            bounds, got = _device(cam, pts, u, w)
            host = _host(cam, p, pts, bounds, u, w)
            assert got.shape == (n, m) and splat_ref.same_records(got, host), (n, m, w is not None, splat_ref.differing(got, host))
            _rows_present(pts, w, bounds, host)
    cam.close()


@pytest.mark.gpu
def test_grid_stride_walk_takes_a_second_trip(gpu):
    cam, p = _camera("C3")
    n, m = STRIDE_SHAPE
    pts, u = pc.batch(p, n), _u(n, m)
    lam = np.resize(pc.wavelengths(10), n).astype(F32)
    for w in (None, lam):
        bounds, got = _device(cam, pts, u, w)
        host = _host(cam, p, pts, bounds, u, w)
        assert splat_ref.same_records(got, host), splat_ref.differing(got, host)
        _rows_present(pts, w, bounds, host)
    cam.close()


@pytest.mark.gpu
def test_refusing_cameras(gpu):
    """lensModel NONE, a pinhole thin lens and a camera outside the domain: every box is empty, every splat kSpNoBox; with a box given
    all the same the trace refuses every ray for the model's reason, on the device as on the host"""
    import torch
    base = pc.params_of("C3")
    pts = pc.points(base)
    u = _u(len(pts), 5)
    box = np.zeros(len(pts), _capi.PUPIL_BOUNDS_DTYPE)
    box["aim"], box["count"], box["lattice"], box["flags"] = (-0.5, -0.25, 0.5, 0.25), 7, 256, 1
    for p in (dict(base, lensModel=_capi.LENS_NONE), dict(pc.params_of("C1"), useDof=False), dict(base, focalLength=-10.0)):
        cam = tc.update(ZoicCamera(device=0), p)
        for lam in (None, pc.wavelengths(len(pts))):
            bounds, got = _device(cam, pts, u, lam)
            assert (got["flags"] == splat_ref.NO_BOX).all() and splat_ref.same_records(got, _host(cam, p, pts, bounds, u, lam))
            forced = cam.splat_points(pts, box, u, lam)          # the numpy path
            assert forced.shape == (len(pts), 5) and splat_ref.same_records(forced, _host(cam, p, pts, box, u, lam))
            assert ((forced["flags"] & 1) == 0).all() and ((forced["flags"] & splat_ref.NO_BOX) == 0).all()
        cam.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_torch_path_counters_and_retry_streams(gpu):
    """a non-default stream, out= reuse, and nothing else of the camera moves: counters() before equals after, and create_rays with
    the same retry-stream states gives the same records after as before"""
    import torch
    cam, p = _camera("C3")
    nr, w, h, spp = 4096, 64, 32, 2
    smp, st = synthetic_samples(nr, w, h, spp), ray_rng_states(nr)
    first = cam.create_rays(smp, rng_states=st)["rays"].copy()
    before = cam.counters()
    n, m = 257, 9
    pts_h, u_h = pc.batch(p, n), _u(n, m)
    lam_h = np.full(n, 550.0, F32)
    side = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(side):
        pts, u, lam = (torch.from_numpy(a).to("cuda:0") for a in (pts_h, u_h, lam_h))
        bounds = cam.pupil_bounds(pts, G)
        out = torch.full((n, m, 8), 7.0, dtype=torch.float32, device="cuda:0")
        res = cam.splat_points(pts, bounds, u, out=out)
        assert res.data_ptr() == out.data_ptr()
        spectral = cam.splat_points(pts, bounds, u, lam, stream=side.cuda_stream)
    side.synchronize()
    assert cam.counters() == before
    b = pupil_bounds_records(bounds)
    assert splat_ref.same_records(splat_records(out), _host(cam, p, pts_h, b, u_h))
    assert splat_ref.same_records(splat_records(spectral), _host(cam, p, pts_h, b, u_h, lam_h))
    with torch.cuda.stream(side):                                  # out= reuse: every record is rewritten
        again = cam.splat_points(pts, bounds, u, lam, out=out)
    side.synchronize()
    assert again.data_ptr() == out.data_ptr() and splat_ref.same_records(splat_records(out), splat_records(spectral))
    with pytest.raises(ValueError):
        cam.splat_points(pts, bounds, u, out=torch.empty((n, m, 7), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        cam.splat_points(pts, bounds[:-1], u)
    with pytest.raises(ValueError):
        cam.splat_points(pts, bounds, u[:, :0])
    rays = cam.create_rays(smp, rng_states=st)["rays"]
    assert first.tobytes() == rays.tobytes()
    cam.close()


@pytest.mark.gpu
def test_argument_errors(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C3")
    n, m = 16, 4
    pts = torch.from_numpy(pc.batch(p, n + 1)).to("cuda:0")
    lam = torch.full((n + 1,), 550.0, dtype=torch.float32, device="cuda:0")
    u = torch.from_numpy(_u(n + 1, m)).to("cuda:0")
    bounds = cam.pupil_bounds(pts, G)
    out = torch.full((n + 1, m, 8), 7.0, dtype=torch.float32, device="cuda:0")
    host = np.zeros((n * m, 8), F32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, B, L, Uu, O = pts.data_ptr(), bounds.data_ptr(), lam.data_ptr(), u.data_ptr(), out.data_ptr()
    d, s = lib.zoic_splat_points_device, lib.zoic_splat_points_spectral_device
    before = cam.counters()
    assert d(cam._h, n, P, B, 0, Uu, O, st) == 1                      # m = 0 with n > 0
    assert s(cam._h, n, P, B, L, 0, Uu, O, st) == 1
    assert d(cam._h, n, None, B, m, Uu, O, st) == 1
    assert d(cam._h, n, P, None, m, Uu, O, st) == 1
    assert d(cam._h, n, P, B, m, None, O, st) == 1
    assert d(cam._h, n, P, B, m, Uu, None, st) == 1
    assert d(cam._h, n, P, B, m, Uu, O + 4, st) == 1                  # d_splats misaligned by 4 bytes
    assert d(cam._h, n, P, B, m, Uu, O + 8, st) == 1
    assert d(cam._h, n, P, B + 8, m, Uu, O, st) == 1                  # d_bounds misaligned
    assert d(cam._h, n, P, B, m, Uu + 4, O, st) == 1                  # d_u misaligned
    assert d(cam._h, n, P + 2, B, m, Uu, O, st) == 1                  # d_points misaligned
    assert d(cam._h, n, P, B, m, Uu, host.ctypes.data, st) == 1       # a host pointer
    assert d(cam._h, n, host.ctypes.data, B, m, Uu, O, st) == 1
    assert d(cam._h, 1 << 40, P, B, 1 << 20, Uu, O, st) == 1          # n m too large
    assert d(None, n, P, B, m, Uu, O, st) == 1
    assert d(cam._h, 0, None, None, m, None, None, st) == 0           # n = 0: no-op
    assert d(cam._h, 0, None, None, 0, None, None, st) == 0
    assert s(cam._h, n, P, B, None, m, Uu, O, st) == 1                # NULL d_wavelengths
    assert s(cam._h, n, P, B, L + 2, m, Uu, O, st) == 1               # misaligned d_wavelengths
    assert s(cam._h, n, P, None, L, m, Uu, O, st) == 1
    assert s(cam._h, n, P, B, L, m, Uu, None, st) == 1
    assert s(cam._h, n, P, B, L, m, Uu, O + 4, st) == 1
    assert s(cam._h, 0, None, None, None, m, None, None, st) == 0
    fresh = ZoicCamera(device=0)
    assert d(fresh._h, n, P, B, m, Uu, O, st) == 9                    # NOT_UPDATED
    assert s(fresh._h, n, P, B, L, m, Uu, O, st) == 9
    fresh.close()
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and cam.counters() == before     # nothing was launched: d_splats is untouched
    assert d(cam._h, n, P, B, m, Uu, O, st) == 0
    torch.cuda.synchronize()
    assert (out[n] == 7.0).all().item()                               # and nothing is written past n m
    hb = pupil_bounds_records(bounds)
    assert splat_ref.same_records(splat_records(out[:n]), _host(cam, p, pts[:n].cpu().numpy(), hb[:n], u[:n].cpu().numpy()))
    cam.close()
    host_cam = tc.update(ZoicCamera(device=-1), pc.params_of("C3"))
    assert d(host_cam._h, n, P, B, m, Uu, O, st) == 11                # a tables-only camera: NO_DEVICE
    assert s(host_cam._h, n, P, B, L, m, Uu, O, st) == 11
    host_cam.close()


@pytest.mark.gpu
def test_the_call_follows_updates_and_new_dispersion(gpu):
    cam, p = _camera("C3")
    cam.set_abbe_numbers(None)
    n, m = 41, 6
    pts, u = pc.batch(p, n), _u(n, m)
    lam = np.resize(pc.wavelengths(10), n).astype(F32)
    b1, first = _device(cam, pts, u)
    assert splat_ref.same_records(first, _host(cam, p, pts, b1, u))
    # another lens
    p2 = pc.params_of("triplet")
    tc.update(cam, p2)
    b2, second = _device(cam, pts, u)
    assert splat_ref.same_records(second, _host(cam, p2, pts, b2, u)) and not splat_ref.same_records(second, first)
    # another dispersion: taken at the call, no update in between.  The same d-line bounds for both, so that only the splats' trace moves
    plain = cam.splat_points(pts, b2, u, lam)
    assert splat_ref.same_records(plain, _host(cam, p2, pts, b2, u, lam))
    cam.set_abbe_numbers(np.full(cam.info()["lensCount"], 25.0, F32))
    flint = cam.splat_points(pts, b2, u, lam)
    assert splat_ref.same_records(flint, _host(cam, p2, pts, b2, u, lam)) and not splat_ref.same_records(flint, plain)
    assert splat_ref.same_records(_device(cam, pts, u)[1], second)     # the d-line call does not read it
    cam.set_abbe_numbers(None)
    # a thin lens, then stopped down
    p3 = pc.params_of("C1-vignetting")
    tc.update(cam, p3)
    b3, third = _device(cam, pts, u, lam)
    assert splat_ref.same_records(third, _host(cam, p3, pts, b3, u, lam))
    p4 = pc.params_of("C3-f8")
    tc.update(cam, p4)
    b4, last = _device(cam, pts, u)
    assert splat_ref.same_records(last, _host(cam, p4, pts, b4, u))
    assert not splat_ref.same_records(last, first)
    cam.close()

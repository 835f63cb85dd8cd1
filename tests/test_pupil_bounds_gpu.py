"""Pupil bounds on the MI355X (zoic_pupil_bounds_device and its spectral form): the kernels -- one scene point per wave, the lattice's
aims spread over the lanes, a cross-lane butterfly -- give the host twin's records bit for bit at every batch shape that takes another
path through the mapping; the call touches no counter and no retry stream; bad arguments are refused before any launch; after an
update or a new dispersion the call follows the new tables.

Host twin: csrc/pupil_bounds.hpp compiled with clang++ (pupil_driver.py), which tests/test_pupil_bounds_cpu.py holds against an
independent restatement.  Cameras and points: pupil_cases.py."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import ZoicCamera, _capi, pupil_bounds_records
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import pupil_cases as pc
import pupil_driver
import pupil_ref
import traceback_cases as tc

# 1: a workgroup with three idle waves; 3: one idle wave; 4: a full workgroup; 5: a partial second workgroup; 257: 64 full
# workgroups and a last one with a single busy wave
SHAPES = (1, 3, 4, 5, 257)
GRID_CAP = 2048   # workgroups of four waves (kPassGridCap, device_pass.hpp; pupil_bounds.hip takes a point per wave): a larger batch is walked with a grid stride


def _camera(name):
    p = pc.params_of(name)
    return tc.update(ZoicCamera(device=0), p), p


def _device(cam, pts, G, window=None, lam=None):
    return cam.pupil_bounds(pts, G, window, lam)


def _host(cam, p, pts, G, window=None, lam=None):
    return pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, G, window, lam, None if lam is None else cam.dispersion())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C3", "C5", "C1-vignetting", "C3-f8"])
def test_kernel_equals_host_twin_bitwise(gpu, name):
    cam, p = _camera(name)
    pts = pc.batch(p, max(SHAPES))
    for G in pc.LATTICES:
        for window in (None, pc.WINDOW):
            host = _host(cam, p, pts, G, window)
            assert (host["count"] > 0).sum() > len(pts) // 4
            for n in SHAPES:
                got = _device(cam, pts[:n], G, window)
                assert got.dtype == pupil_ref.DTYPE and got.shape == (n,)
                assert pupil_ref.same_records(got, host[:n]), (G, window, n)
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C3", "triplet", "C1"])
def test_spectral_kernel_equals_host_twin_bitwise(gpu, name):
    cam, p = _camera(name)
    if name in bs.DISPERSIVE:
        bs.set_dispersion(cam, name)
    pts = pc.batch(p, max(SHAPES))
    lam = np.resize(pc.wavelengths(10), len(pts)).astype(np.float32)
    for G in pc.LATTICES:
        host = _host(cam, p, pts, G, pc.WINDOW if G == 16 else None, lam)
        bad = lam == np.float32(pc.BAD_LAMBDA)
        assert bad.any() and (host["count"][bad] == 0).all() and (host["flags"][bad] == 1 << (16 + bs.TB_WAVELENGTH)).all()
        for n in SHAPES:
            got = _device(cam, pts[:n], G, pc.WINDOW if G == 16 else None, lam[:n])
            assert pupil_ref.same_records(got, host[:n]), (G, n)
    if p["lensModel"] == _capi.RAYTRACED:
        assert not pupil_ref.same_records(_host(cam, p, pts, 16, None, lam), _host(cam, p, pts, 16))
    cam.close()


@pytest.mark.gpu
def test_grid_stride_walk_takes_a_second_slab(gpu):
    cam, p = _camera("C3")
    n = 4 * GRID_CAP + 1
    pts = pc.batch(p, n)
    assert pupil_ref.same_records(_device(cam, pts, 8), _host(cam, p, pts, 8))
    lam = np.resize(pc.wavelengths(10), n).astype(np.float32)
    assert pupil_ref.same_records(_device(cam, pts, 8, pc.WINDOW, lam), _host(cam, p, pts, 8, pc.WINDOW, lam))
    cam.close()


@pytest.mark.gpu
def test_refusing_cameras(gpu):
    """lensModel NONE, a pinhole thin lens and a camera outside the domain: count = 0 with the reason's bit, on the device as on the host"""
    base = pc.params_of("C3")
    pts = pc.points(base)
    for p in (dict(base, lensModel=_capi.LENS_NONE), dict(pc.params_of("C1"), useDof=False), dict(base, focalLength=-10.0)):
        cam = tc.update(ZoicCamera(device=0), p)
        for lam in (None, pc.wavelengths(len(pts))):
            got = _device(cam, pts, 16, None, lam)
            assert (got["count"] == 0).all() and ((got["flags"] & 1) == 0).all() and (got["flags"] != 0).all()
            assert pupil_ref.same_records(got, _host(cam, p, pts, 16, None, lam))
        cam.close()


@pytest.mark.gpu
def test_counters_and_retry_streams_are_untouched(gpu):
    import torch
    cam, p = _camera("C3")
    n, w, h, spp = 4096, 64, 32, 2
    smp, st = synthetic_samples(n, w, h, spp), ray_rng_states(n)
    first = cam.create_rays(smp, rng_states=st)["rays"].copy()
    before = cam.counters()
    pts = torch.from_numpy(pc.batch(p, 257)).to("cuda:0")
    lam = torch.full((257,), 550.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((257, 12), 7.0, dtype=torch.float32, device="cuda:0")
    res = cam.pupil_bounds(pts, 16, pc.WINDOW, out=out)
    assert res.data_ptr() == out.data_ptr()
    spectral = cam.pupil_bounds(pts, 16, pc.WINDOW, lam)
    torch.cuda.synchronize()
    assert cam.counters() == before
    host = _host(cam, p, pts.cpu().numpy(), 16, pc.WINDOW)
    assert pupil_ref.same_records(pupil_bounds_records(out), host)
    assert pupil_ref.same_records(pupil_bounds_records(spectral), _host(cam, p, pts.cpu().numpy(), 16, pc.WINDOW, lam.cpu().numpy()))
    again = cam.create_rays(smp, rng_states=st)["rays"]
    assert first.tobytes() == again.tobytes()
    cam.close()


@pytest.mark.gpu
def test_argument_errors(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C3")
    n = 64
    pts = torch.from_numpy(pc.batch(p, n + 1)).to("cuda:0")
    lam = torch.full((n + 1,), 550.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((n + 1, 12), 7.0, dtype=torch.float32, device="cuda:0")
    host = np.zeros((n, 12), np.float32)
    win = (C.c_float * 4)(*pc.WINDOW)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, L, O = pts.data_ptr(), lam.data_ptr(), out.data_ptr()
    d, s = lib.zoic_pupil_bounds_device, lib.zoic_pupil_bounds_spectral_device
    before = cam.counters()
    assert d(cam._h, n, None, 16, None, O, st) == 1
    assert d(cam._h, n, P, 16, None, None, st) == 1
    assert d(cam._h, n, P, 16, win, O + 4, st) == 1                   # d_bounds misaligned by 4 bytes
    assert d(cam._h, n, P, 16, None, O + 8, st) == 1
    assert d(cam._h, n, P + 2, 16, None, O, st) == 1                  # d_points misaligned
    assert d(cam._h, n, P, 16, None, host.ctypes.data, st) == 1       # a host pointer
    assert d(cam._h, n, host.ctypes.data, 16, None, O, st) == 1
    for G in (0, 4, 12, 24, 64, -16):
        assert d(cam._h, n, P, G, None, O, st) == 1                   # a lattice that is not 8, 16 or 32
        assert s(cam._h, n, P, L, G, win, O, st) == 1
    assert d(None, n, P, 16, None, O, st) == 1
    assert d(cam._h, 0, None, 16, None, None, st) == 0                # n = 0: no-op
    assert s(cam._h, n, P, None, 16, None, O, st) == 1                # NULL d_wavelengths
    assert s(cam._h, n, P, L + 2, 16, None, O, st) == 1               # misaligned d_wavelengths
    assert s(cam._h, n, None, L, 16, None, O, st) == 1
    assert s(cam._h, n, P, L, 16, None, None, st) == 1
    assert s(cam._h, n, P, L, 16, win, O + 4, st) == 1
    assert s(cam._h, 0, None, None, 16, None, None, st) == 0
    fresh = ZoicCamera(device=0)
    assert d(fresh._h, n, P, 16, None, O, st) == 9                    # NOT_UPDATED
    assert s(fresh._h, n, P, L, 16, None, O, st) == 9
    fresh.close()
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and cam.counters() == before     # nothing was launched: d_bounds is untouched
    assert d(cam._h, n, P, 16, win, O, st) == 0
    torch.cuda.synchronize()
    assert (out[n] == 7.0).all().item()                               # and nothing is written past n
    assert pupil_ref.same_records(pupil_bounds_records(out[:n]), _host(cam, p, pts[:n].cpu().numpy(), 16, pc.WINDOW))
    cam.close()
    host_cam = tc.update(ZoicCamera(device=-1), pc.params_of("C3"))
    assert d(host_cam._h, n, P, 16, None, O, st) == 11                # a tables-only camera: NO_DEVICE
    assert s(host_cam._h, n, P, L, 16, None, O, st) == 11
    host_cam.close()


@pytest.mark.gpu
def test_the_call_follows_updates_and_new_dispersion(gpu):
    cam, p = _camera("C3")
    pts = pc.batch(p, 41)
    lam = np.resize(pc.wavelengths(10), len(pts)).astype(np.float32)
    first = _device(cam, pts, 16)
    assert pupil_ref.same_records(first, _host(cam, p, pts, 16))
    wide_open = _host(cam, p, pts, 32)
    # another lens
    p2 = pc.params_of("triplet")
    tc.update(cam, p2)
    second = _device(cam, pts, 16)
    assert pupil_ref.same_records(second, _host(cam, p2, pts, 16)) and not pupil_ref.same_records(second, first)
    # another dispersion: taken at the call, no update in between
    plain = _device(cam, pts, 16, None, lam)
    assert pupil_ref.same_records(plain, _host(cam, p2, pts, 16, None, lam))
    cam.set_abbe_numbers(np.full(cam.info()["lensCount"], 25.0, np.float32))
    flint = _device(cam, pts, 16, None, lam)
    assert pupil_ref.same_records(flint, _host(cam, p2, pts, 16, None, lam)) and not pupil_ref.same_records(flint, plain)
    assert pupil_ref.same_records(_device(cam, pts, 16), second)      # the d-line call does not read it
    cam.set_abbe_numbers(None)
    # a thin lens, then stopped down
    p3 = pc.params_of("C1-vignetting")
    tc.update(cam, p3)
    assert pupil_ref.same_records(_device(cam, pts, 8, pc.WINDOW), _host(cam, p3, pts, 8, pc.WINDOW))
    p4 = pc.params_of("C3-f8")
    tc.update(cam, p4)
    last = _device(cam, pts, 32)
    assert pupil_ref.same_records(last, _host(cam, p4, pts, 32)) and (last["count"] < wide_open["count"]).any()
    cam.close()

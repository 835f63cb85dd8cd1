"""Reverse projection on the MI355X (zoic_project_points_device): the batch kernel gives zoic_project_point's bits, flags included,
deterministically and whatever the batch size; projected points land where the forward rays of their sample meet (Kolb) or pass
(thin lens); the opt-in switch and the error codes behave as the header states."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states

from reverse_ref import kolb_point_set, thin_point_set

SLAB = 2048 * 256   # one grid of the kernel (kPassGridCap x kPassBlock, device_pass.hpp): larger batches are walked slab by slab


def _camera(cfg, **over):
    p = camera_params(cfg)
    p.update(over)
    cam = ZoicCamera(device=0)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    cam.set_precision(PRECISION_STRICT)
    cam.update(**p)
    return cam, p


def _points(cam, p):
    info = cam.info()
    if p["lensModel"] == _capi.THINLENS:
        pts = [thin_point_set(float(info["tan_fov"]), fd)[0] for fd in (p["focalDistance"], 30.0)]
    else:
        pts = [kolb_point_set(info, p["sensorWidth"], p["focalDistance"])[0]]
    rng = np.random.default_rng(7)   # and points anywhere: behind, beside, far out, edge values
    wild = rng.normal(0.0, 1.0, (4096, 3)).astype(np.float32) * np.float32([50.0, 50.0, 200.0])
    edge = np.array([[0, 0, -10], [0, 0, 10], [np.nan, 0, -1], [0, np.inf, -1], [1e30, 1e30, -1e30], [1e-30, 0, -1], [-0.0, -0.0, -1]],
                    np.float32)
    return np.ascontiguousarray(np.concatenate(pts + [wild, edge]), dtype=np.float32)


def _host(cam, pts):
    out = np.array([cam.project_point(q) for q in pts])
    return out[:, :2].astype(np.float32), out[:, 2].astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_batch_equals_host_bitwise(gpu, cfg):
    import torch
    cam, p = _camera(cfg)
    pts = _points(cam, p)
    scr, fl = cam.project_points(pts)
    hs, hf = _host(cam, pts)
    assert np.array_equal(scr.view(np.uint32), hs.view(np.uint32))
    assert np.array_equal(fl.astype(np.uint32), hf)
    assert (hf & 1).sum() > len(pts) // 2
    # twice: the same bits; then n = 1, 777 and more than one slab (tiled), each a prefix / tiling of the same points
    scr2, fl2 = cam.project_points(pts)
    assert np.array_equal(scr2.view(np.uint32), scr.view(np.uint32)) and np.array_equal(fl2, fl)
    for n in (1, 777):
        s, f = cam.project_points(pts[:n])
        assert np.array_equal(s.view(np.uint32), scr[:n].view(np.uint32)) and np.array_equal(f, fl[:n])
    reps = SLAB // len(pts) + 2
    big = torch.from_numpy(np.tile(pts, (reps, 1))).to("cuda:0")
    s, f = cam.project_points(big)
    torch.cuda.synchronize()
    assert big.shape[0] > SLAB
    assert np.array_equal(s.cpu().numpy().view(np.uint32), np.tile(scr, (reps, 1)).view(np.uint32))
    assert np.array_equal(f.cpu().numpy(), np.tile(fl, reps))
    cam.close()


def _meeting_point(o, d):
    """least-squares point closest to the lines o + t d (rows)"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    A = np.zeros((3, 3))
    b = np.zeros(3)
    for oi, di in zip(o, d):
        M = np.eye(3) - np.outer(di, di)
        A += M
        b += M @ oi
    return np.linalg.solve(A, b)


# |project_points(W) - s0| of the least-squares meeting point W of 4096 forward rays at s0 (the retry streams of ray_rng_states(n, 1)),
# measured on the CPU with the oracle, whose records are the STRICT kernel's for these streams, and the host projection: at most
# C2 7.4e-5, C3 4.7e-4, C5 3.6e-4 over this lattice (the rays of an aberrated lens do not meet in one point: W is the centre of the
# blur, not a point of the chief ray).  Tolerances: twice that.  (C5 vignettes the outer samples entirely: they are skipped.)
S0 = [(0.0, 0.3), (0.3, 0.0), (-0.5, 0.2), (0.6, -0.4), (-0.2, -0.7), (0.8, 0.3), (0.1, 0.1), (-0.15, 0.05), (0.05, -0.2)]
FORWARD_TOL = {"C2": 1.5e-4, "C3": 9.4e-4, "C5": 7.2e-4}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C2", "C3", "C5"])
def test_kolb_projection_matches_forward_rays(gpu, cfg):
    cam, p = _camera(cfg)
    rng = np.random.default_rng(3)
    worst = 0.0
    checked = 0
    for s0 in S0:
        n = 4096
        smp = np.zeros((n, 4), np.float32)
        smp[:, 0], smp[:, 1] = s0
        smp[:, 2:] = rng.random((n, 2), dtype=np.float32)
        r = cam.create_rays(smp, rng_states=ray_rng_states(n, seed=1))
        live = r["weight"] > 0
        if live.sum() < 256:
            continue
        W = _meeting_point(r["origin"][:, live].T.astype(np.float64), r["dir"][:, live].T.astype(np.float64))
        sx, sy, f = cam.project_point(W.astype(np.float32))
        scr, fl = cam.project_points(W.astype(np.float32)[None, :])
        assert f & 1 and fl[0] == f and (scr[0, 0], scr[0, 1]) == (np.float32(sx), np.float32(sy))
        err = max(abs(sx - s0[0]), abs(sy - s0[1]))
        worst = max(worst, err)
        checked += 1
    assert checked >= 3
    assert worst <= FORWARD_TOL[cfg], worst
    cam.close()


@pytest.mark.gpu
def test_thin_lens_rays_pass_through_projected_point(gpu):
    cam, p = _camera("C1", useDof=True)
    fd = p["focalDistance"]
    rng = np.random.default_rng(11)
    Po = np.stack([rng.uniform(-30, 30, 16), rng.uniform(-20, 20, 16), np.full(16, -fd)], 1).astype(np.float32)
    scr, fl = cam.project_points(Po)
    assert (fl == 1).all()
    for q, s in zip(Po.astype(np.float64), scr):
        smp = np.zeros((1024, 4), np.float32)
        smp[:, 0], smp[:, 1] = s
        smp[:, 2:] = rng.random((1024, 2), dtype=np.float32)
        r = cam.create_rays(smp)
        o, d = r["origin"].T.astype(np.float64), r["dir"].T.astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        v = q - o
        dist = np.linalg.norm(v - (v * d).sum(1, keepdims=True) * d, axis=1)
        assert dist.max() <= 1e-5 * np.linalg.norm(q), dist.max()
    cam.close()


@pytest.mark.gpu
def test_switch_errors_and_independence(gpu):
    import torch
    lib = _capi.load()
    a, p = _camera("C2")
    b, _ = _camera("C2")
    q = (0.4, -0.2, -100.0)
    assert a.reverse_ray(q) is False and b.reverse_ray(q) is False
    b.set_reverse_projection(True)
    assert b.reverse_ray(q) is True and a.reverse_ray(q) is False     # a second camera's switch leaves the first alone
    po = _capi.Vec3(*q)
    ps = (C.c_float * 2)()
    t = C.c_float(5.0)
    assert lib.zoic_camera_reverse_ray(b._h, C.byref(po), C.c_float(0.3), ps, C.byref(t)) == 1
    sx, sy, f = b.project_point(q)
    assert (ps[0], ps[1]) == (np.float32(sx), np.float32(sy)) and t.value == 5.0
    # the batch call works whatever the switch says
    s1, f1 = a.project_points(np.array([q], np.float32))
    assert (s1[0, 0], s1[0, 1], int(f1[0])) == (np.float32(sx), np.float32(sy), f)
    dev = torch.zeros((8, 3), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((8, 2), dtype=torch.float32, device="cuda:0")
    host = np.zeros((8, 3), np.float32)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.zoic_project_points_device(a._h, 8, None, out.data_ptr(), None, C.c_void_p(st)) == 1
    assert lib.zoic_project_points_device(a._h, 8, dev.data_ptr(), None, None, C.c_void_p(st)) == 1
    assert lib.zoic_project_points_device(a._h, 8, host.ctypes.data, out.data_ptr(), None, C.c_void_p(st)) == 1   # not device memory
    assert lib.zoic_project_points_device(a._h, 8, dev.data_ptr() + 2, out.data_ptr(), None, C.c_void_p(st)) == 1  # misaligned
    assert lib.zoic_project_points_device(a._h, 0, None, None, None, C.c_void_p(st)) == 0                           # n = 0: no-op
    assert lib.zoic_project_points_device(a._h, 8, dev.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 0      # flags may be NULL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()   # the origin is behind the lens: (+0, +0)
    fresh = ZoicCamera(device=0)
    assert lib.zoic_project_points_device(fresh._h, 8, dev.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 9   # NOT_UPDATED
    fresh.close()
    a.close()
    b.close()

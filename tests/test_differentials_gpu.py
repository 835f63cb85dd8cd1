"""Traced ray differentials on the MI355X (zoic_ray_differentials_device, zoic_create_rays_arnold_differentials): the rays are
unchanged, the derivatives agree with finite differences of a restatement checked against the oracle, the pass is deterministic
and mode-independent, zeros where there is no ray, error codes as the header states."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import CONFIGS, ray_rng_states

from device_cases import camera as _camera, oracle as _oracle, params as _params, samples as _samples
from differentials_ref import kolb_jacobian_fd, kolb_start, rel_err, surfaces, thin_jacobian_fd, trace

N = 1 << 16


def _rays_and_diffs(cam, s_np, **kw):
    import torch
    s = torch.from_numpy(s_np).cuda()
    rays = cam.create_rays(s, **kw)["rays"]
    d = cam.ray_differentials(s, rays, **kw)
    torch.cuda.synchronize()
    return rays.cpu().numpy(), d.cpu().numpy()


def _arnold_inputs(s_np, dsx=1.0, dsy=1.0):
    n = len(s_np)
    a = np.zeros((n, 7), np.float32)
    a[:, 0], a[:, 1], a[:, 4], a[:, 5] = s_np[:, 0], s_np[:, 1], s_np[:, 2], s_np[:, 3]
    a[:, 2], a[:, 3] = dsx, dsy
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
@pytest.mark.parametrize("precision", [PRECISION_STRICT, PRECISION_FAST])
def test_arnold_rows_unchanged(gpu, cfg, precision):
    """origin, dir and weight of every row are zoic_create_rays_arnold's, bit for bit; the derivative fields are the batch call's --
    at the full size and at n = 257 (a partial last wave and a second wave-tile)"""
    import torch
    p = _params(cfg)
    cam = _camera(p, precision)
    rs = np.random.RandomState(3)
    dsx, dsy = rs.uniform(-2e-3, 2e-3, N).astype(np.float32), rs.uniform(-2e-3, 2e-3, N).astype(np.float32)
    for n in (N, 257):
        s = _samples(N)[:n]
        inputs = _arnold_inputs(s)
        plain = cam.create_rays_arnold(inputs, ray_index_base=7)
        rows = cam.create_rays_arnold(inputs, ray_index_base=7, differentials=True)
        assert rows.shape[0] == n
        keep = np.r_[0:6, 18:21]
        assert np.array_equal(rows[:, keep].view(np.uint32), plain[:, keep].view(np.uint32))
        st = torch.from_numpy(s).cuda()
        rays = cam.create_rays(st, ray_index_base=7)["rays"]
        d = cam.ray_differentials(st, rays, ray_index_base=7).cpu().numpy()
        assert np.array_equal(rows[:, 6:18].view(np.uint32), d.view(np.uint32))
        # per-row dsx / dsy scale the raw columns
        inputs2 = inputs.copy()
        inputs2[:, 2] = dsx[:n]
        inputs2[:, 3] = dsy[:n]
        rows2 = cam.create_rays_arnold(inputs2, ray_index_base=7, differentials=True)
        live = rows[:, 18] != 0
        for cols, k in ((slice(6, 9), 2), (slice(9, 12), 3), (slice(12, 15), 2), (slice(15, 18), 3)):
            want = (rows[:, cols] * inputs2[:, k:k + 1]).astype(np.float32)
            got = rows2[:, cols]
            ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert ulps[live].max(initial=0) <= 1
    cam.close()


def _check_kolb(cam, oc, p, s, diffs, rays, states, oracle_lib, need_retried=1000):
    w = rays[:, 6]
    flags = rays[:, 7].view(np.uint32)
    tries = ((flags >> 1) & 31).astype(np.int64)
    live = np.nonzero(w != 0)[0]
    retried = int((tries[live] > 0).sum())
    assert retried >= need_retried, "only %d retried live rays" % retried
    o0, d0 = kolb_start(oc, p, s[live], tries[live], states[live], oracle_lib)
    surf = surfaces(oc.lens_table())
    # the restatement reproduces the rays the GPU (== the oracle, STRICT) made
    ro, rd = trace(surf, o0, d0)
    eo = np.linalg.norm(-ro - rays[live, 0:3], axis=1) / np.linalg.norm(rays[live, 0:3], axis=1)
    ed = np.linalg.norm(-rd - rays[live, 3:6], axis=1) / np.linalg.norm(rays[live, 3:6], axis=1)
    assert np.median(eo) < 1e-5 and np.median(ed) < 1e-5 and np.percentile(ed, 99.9) < 1e-4, (np.median(eo), np.median(ed))
    hs = np.float32(np.float32(p["sensorWidth"]) * np.float32(0.5))
    e = rel_err(diffs[live], kolb_jacobian_fd(surf, hs, o0, d0))
    assert np.median(e) <= 1e-5 and (e <= 1e-3).mean() >= 0.999, (float(np.median(e)), float((e <= 1e-3).mean()))
    return live


KOLB_CASES = [("C2", {}), ("C3", {}), ("C4", {}), ("C5", {}), ("C2", dict(kolbSamplingLUT=False))]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,over", KOLB_CASES, ids=["C2", "C3", "C4", "C5", "C2-noLUT"])
def test_kolb_differentials_correct(gpu, oracle_lib, cfg, over):
    p = _params(cfg, **over)
    cam = _camera(p)
    oc = _oracle(oracle_lib, p)
    s = _samples(N)
    states = ray_rng_states(N, seed=1)
    rays, diffs = _rays_and_diffs(cam, s)
    ref = oc.create_rays(s, rng_states=states)
    assert np.array_equal(rays[:, 7].view(np.uint32).astype(np.uint8), ref["flags"])
    assert np.array_equal(rays[:, 0:7].T.view(np.uint32), ref["planes"].view(np.uint32))
    live = _check_kolb(cam, oc, p, s, diffs, rays, states, oracle_lib)
    assert np.isfinite(diffs[live]).all()
    dead = rays[:, 6] == 0
    assert dead.any() or cfg != "C5"
    assert not diffs[dead].view(np.uint32).any()   # +0.0 in all 12 floats
    cam.close()


THIN_CASES = [("C1", {}), ("C1", dict(opticalVignettingDistance=5.0)),
              ("C1", dict(opticalVignettingDistance=5.0, useImage=True, bokehPath="procedural:hexagon256")), ("C1", dict(useDof=False))]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,over", THIN_CASES, ids=["C1", "C1-vignet", "C1-vignet-image", "C1-noDOF"])
def test_thin_differentials_correct(gpu, oracle_lib, cfg, over):
    p = _params(cfg, **over)
    cam = _camera(p)
    oc = _oracle(oracle_lib, p)
    s = _samples(N)
    rays, diffs = _rays_and_diffs(cam, s)
    ref = oc.create_rays(s, rng_states=ray_rng_states(N, seed=1))
    assert np.array_equal(rays[:, 0:7].T.view(np.uint32), ref["planes"].view(np.uint32))
    tries = (rays[:, 7].view(np.uint32) >> 1) & 31
    if p["opticalVignettingDistance"] > 0:
        assert (tries[rays[:, 6] != 0] > 0).sum() >= 1000
    live = rays[:, 6] != 0
    tl = oc.thinlens()
    fd = thin_jacobian_fd(s[live, 0], s[live, 1], float(tl["tan_fov"]), rays[live, 0:3], p["focalDistance"], bool(p["useDof"]))
    e = rel_err(diffs[live], fd)[:, 2:]
    assert np.median(e) <= 1e-5 and (e <= 1e-3).mean() >= 0.999, (float(np.median(e)), float((e <= 1e-3).mean()))
    assert not diffs[live][:, 0:6].view(np.uint32).any()   # dO = 0: the lens point is held fixed
    assert not diffs[~live].view(np.uint32).any()
    # the oracle's own rays, differenced in f32 (first-try rays whose neighbours also take their first try)
    h = np.float32(1e-3)
    sp, sm = s.copy(), s.copy()
    sp[:, 0] += h
    sm[:, 0] -= h
    rp = oc.create_rays(sp, rng_states=ray_rng_states(N, seed=1))
    rm = oc.create_rays(sm, rng_states=ray_rng_states(N, seed=1))
    ok = live & (tries == 0) & (rp["tries"] == 0) & (rm["tries"] == 0)
    fd32 = (rp["dir"][:, ok] - rm["dir"][:, ok]).T.astype(np.float64) / (np.float64(sp[ok, 0]) - np.float64(sm[ok, 0]))[:, None]
    e32 = np.linalg.norm(diffs[ok, 6:9] - fd32, axis=1) / np.linalg.norm(fd32, axis=1)
    assert ok.sum() > 1000 and np.median(e32) <= 2e-2
    cam.close()


@pytest.mark.gpu
def test_lut_off_matches_oracle_f32_differences(gpu, oracle_lib):
    """Without the LUT a first try's L is the lens sample times the rear aperture, whatever (sx, sy): the oracle's own rays at
    sx +- h (first tries on all three) differenced in f32 are the traced dDdx / dOdx"""
    p = _params("C2", kolbSamplingLUT=False)
    cam = _camera(p)
    oc = _oracle(oracle_lib, p)
    s = _samples(N)
    states = ray_rng_states(N, seed=1)
    rays, diffs = _rays_and_diffs(cam, s)
    h = np.float32(1e-3)
    sp, sm = s.copy(), s.copy()
    sp[:, 0] += h
    sm[:, 0] -= h
    rp, rm = oc.create_rays(sp, rng_states=states), oc.create_rays(sm, rng_states=states)
    tries = (rays[:, 7].view(np.uint32) >> 1) & 31
    ok = (rays[:, 6] != 0) & (tries == 0) & (rp["tries"] == 0) & (rm["tries"] == 0)
    den = (np.float64(sp[ok, 0]) - np.float64(sm[ok, 0]))[:, None]
    for cols, key in ((slice(0, 3), "origin"), (slice(6, 9), "dir")):
        fd = (rp[key][:, ok] - rm[key][:, ok]).T.astype(np.float64) / den
        got = diffs[ok][:, slice(0, 3) if key == "origin" else slice(6, 9)]
        e = np.linalg.norm(got - fd, axis=1) / np.linalg.norm(fd, axis=1)
        assert ok.sum() > 1000 and np.median(e) <= 2e-2, (key, float(np.median(e)))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_deterministic_and_mode_independent(gpu, cfg):
    import torch
    p = _params(cfg)
    s_np = _samples(N)
    a = _camera(p, PRECISION_STRICT)
    b = _camera(p, PRECISION_FAST)
    ra, da = _rays_and_diffs(a, s_np)
    rb, db = _rays_and_diffs(b, s_np)
    same = ra[:, 7].view(np.uint32) == rb[:, 7].view(np.uint32)
    assert same.mean() >= 0.9999
    assert np.array_equal(da[same].view(np.uint32), db[same].view(np.uint32))
    # one call == two calls split by ray_index_base; caller-supplied streams == derived ones
    s = torch.from_numpy(s_np).cuda()
    rays = torch.from_numpy(ra).cuda()
    h = N // 2 + 37
    d1 = a.ray_differentials(s[:h].contiguous(), rays[:h].contiguous(), ray_index_base=0)
    d2 = a.ray_differentials(s[h:].contiguous(), rays[h:].contiguous(), ray_index_base=h)
    assert np.array_equal(torch.cat([d1, d2]).cpu().numpy().view(np.uint32), da.view(np.uint32))
    st = torch.from_numpy(ray_rng_states(N, seed=1).view(np.int32)).cuda()
    d3 = a.ray_differentials(s, rays, rng_states=st)
    assert np.array_equal(d3.cpu().numpy().view(np.uint32), da.view(np.uint32))
    d4 = a.ray_differentials(s, rays, dsx=0.5, dsy=-0.25).cpu().numpy()
    live = ra[:, 6] != 0
    assert np.array_equal(d4[live][:, np.r_[0:3, 6:9]], (da[live][:, np.r_[0:3, 6:9]] * np.float32(0.5)).astype(np.float32))
    assert np.array_equal(d4[live][:, np.r_[3:6, 9:12]], (da[live][:, np.r_[3:6, 9:12]] * np.float32(-0.25)).astype(np.float32))
    a.close()
    b.close()


@pytest.mark.gpu
def test_zeros_and_hostile_samples(gpu):
    import torch
    special = np.array([0.0, -0.0, 1.0, 1e-40, -1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.5, 2.0, -3.0], np.float32)
    rs = np.random.RandomState(9)
    for p in (_params("C5"), _params("C2", kolbSamplingLUT=False), _params("C1", opticalVignettingDistance=5.0),
              _params("C3")):
        cam = _camera(p)
        s = _samples(N)
        hostile = rs.rand(N, 4) < 0.2
        s[hostile] = special[rs.randint(len(special), size=int(hostile.sum()))]
        rays, d = _rays_and_diffs(cam, s)
        dead = rays[:, 6] == 0
        assert not d[dead].view(np.uint32).any()
        plain = ~hostile.any(1) & ~dead
        assert np.isfinite(d[plain]).mean() > 0.999
        cam.close()
    # lensModel NONE: no ray, all-zero differentials
    cam = _camera(_params("C2"))
    s = torch.from_numpy(_samples(4096)).cuda()
    rays = cam.create_rays(s)["rays"]
    cam.update(**_params("C2", lensModel=2))
    out = torch.full((4096, 12), 7.0, device=s.device)
    cam.ray_differentials(s, rays, out=out)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().view(np.uint32).any()
    cam.close()


@pytest.mark.gpu
def test_error_codes(gpu):
    import torch
    lib = gpu
    cam = ZoicCamera(device=0)
    s = torch.zeros((64, 4), device="cuda")
    r = torch.zeros((64, 8), device="cuda")
    o = torch.zeros((64, 12), device="cuda")
    st = C.c_void_p(0)
    assert lib.zoic_ray_differentials_device(cam._h, 64, s.data_ptr(), None, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr(), st) == 9
    rows_in = (np.zeros((4, 7), np.float32))
    rows_out = np.zeros((4, 21), np.float32)
    assert lib.zoic_create_rays_arnold_differentials(cam._h, 4, rows_in.ctypes.data_as(C.POINTER(_capi.CameraInput)),
                                                     rows_out.ctypes.data_as(C.POINTER(_capi.CameraOutput)), 0) == 9
    cam.update(**_params("C2"))
    f = lib.zoic_ray_differentials_device
    assert f(cam._h, 0, None, None, 0, None, 1.0, 1.0, None, st) == 0
    assert f(cam._h, 64, None, None, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr(), st) == 1
    assert f(cam._h, 64, s.data_ptr() + 4, None, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr(), st) == 1
    assert f(cam._h, 64, s.data_ptr(), s.data_ptr() + 8, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr(), st) == 1
    assert f(cam._h, 64, s.data_ptr(), None, 0, None, 1.0, 1.0, o.data_ptr(), st) == 1
    assert f(cam._h, 64, s.data_ptr(), None, 0, r.data_ptr(), 1.0, 1.0, None, st) == 1
    assert f(cam._h, 64, s.data_ptr(), None, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr() + 4, st) == 1
    assert f(None, 64, s.data_ptr(), None, 0, r.data_ptr(), 1.0, 1.0, o.data_ptr(), st) == 1
    assert lib.zoic_create_rays_arnold_differentials(cam._h, 4, None, None, 0) == 1
    with pytest.raises(ValueError):
        cam.ray_differentials(s, r[:10])
    cam.close()


@pytest.mark.gpu
def test_c2_full_frame(gpu, oracle_lib):
    """16.6 M rays: every live ray's differentials are finite; 64 Ki random rays of the frame agree with the restatement"""
    import torch
    cfg = "C2"
    c = CONFIGS[cfg]
    n = c["width"] * c["height"] * c["spp"]
    p = _params(cfg)
    cam = _camera(p)
    s = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1)
    rays = cam.create_rays(s)["rays"]
    d = cam.ray_differentials(s, rays)
    torch.cuda.synchronize()
    live = rays[:, 6] != 0
    assert bool(torch.isfinite(d[live]).all())
    idx = np.sort(np.random.RandomState(1).choice(n, N, replace=False))
    it = torch.from_numpy(idx).cuda()
    s_np, r_np, d_np = s[it].cpu().numpy(), rays[it].cpu().numpy(), d[it].cpu().numpy()
    states = ray_rng_states(n, seed=1)[idx]
    oc = _oracle(oracle_lib, p)
    _check_kolb(cam, oc, p, s_np, d_np, r_np, states, oracle_lib, need_retried=100)
    cam.close()

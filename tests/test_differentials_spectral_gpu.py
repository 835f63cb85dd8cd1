"""Traced ray differentials of spectral records on the MI355X (zoic_ray_differentials_spectral_device): both outputs agree with the
f64 reference started from the records' own tries, the identities the header promises hold bit for bit, rows without a ray or without
a wavelength get +0.0, the error codes are the header's, and the kernel gives the host build's result.

Sizes: 1, 63, 65, 4096 and 524 353 = 2048 x 256 + 65 rays, the first size at which the grid-stride loop takes a second turn and that turn
ends in a partial wave."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import ray_rng_states

import differentials_ref as dref
import differentials_spectral_ref as sref
import host_drivers
from device_cases import BIG, bits as _bits, camera as _camera, oracle as _oracle, params as _params, samples as _samples, spectral_run as _run
from host_drivers import run_differentials_spectral as run_driver
from spectral_ref import BAD, LAMBDA_D32, WAVES

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 63, 65, 4096, BIG]


def _abbe(p, V):
    if V is None:
        return None
    return np.full(ZoicCamera(device=-1).update(**dict(p, useImage=False)).info()["lensCount"], V, F32)


CASES = [("C2", {}, None, False), ("C3", {}, 50.0, False), ("C5", {}, None, True), ("C2", dict(kolbSamplingLUT=False), None, False)]
IDS = ["C2", "C3-V50", "C5-own-streams", "C2-noLUT"]
_CHECKED = {}


def _checked(gpu, oracle_lib, case):
    """One launch of BIG rays per case (STRICT, WAVES cycled over the rays); 64 Ki of them -- the last 129 rows among them -- against
    the f64 reference started from differentials_ref.kolb_start on the records' tries.  Returns the measured figures."""
    if case in _CHECKED:
        return _CHECKED[case]
    cfg, over, V, own = CASES[case]
    p = _params(cfg, **over)
    cam = _camera(p, PRECISION_STRICT, _abbe(p, V))
    disp = cam.dispersion()
    s = _samples(BIG, seed=7)
    lam = np.resize(WAVES, BIG)
    states = ray_rng_states(BIG, seed=3 if own else 1)   # seed 1: the streams the library derives itself
    rays, diffs, chroma = _run(cam, s, lam, states=states if own else None)
    cam.close()
    idx = np.unique(np.r_[np.random.RandomState(1).choice(BIG, 1 << 16, replace=False), BIG - 129:BIG])
    w = rays[idx, 6]
    tries = ((rays[idx, 7].view(np.uint32) >> 1) & 31).astype(np.int64)
    live = idx[w != 0]
    tl = tries[w != 0]
    assert int((tl > 0).sum()) >= 1000, "only %d retried live rays" % int((tl > 0).sum())
    oc = _oracle(oracle_lib, p)
    o0, d0 = dref.kolb_start(oc, p, s[live], tl, states[live], oracle_lib)
    surf = dref.surfaces(oc.lens_table())
    hs = F32(F32(p["sensorWidth"]) * F32(0.5))
    eta = sref.cauchy_eta(disp, lam[live])
    # the restatement reproduces the records (== the oracle on the per-wavelength table, STRICT: tests/test_spectral_gpu.py)
    ro, rd, _ = sref.trace(surf, eta, o0, d0)
    eo = np.linalg.norm(-ro - rays[live, 0:3], axis=1) / np.linalg.norm(rays[live, 0:3], axis=1)
    ed = np.linalg.norm(-rd - rays[live, 3:6], axis=1) / np.linalg.norm(rays[live, 3:6], axis=1)
    assert dref.restatement_holds(eo, ed), (float(np.median(eo)), float(np.median(ed)))
    e = dref.rel_err(diffs[live], sref.jacobian_fd(surf, disp, lam[live], hs, o0, d0))
    fd = sref.wavelength_fd(surf, disp, lam[live], o0, d0)
    el = sref.rel_err_floor(chroma[live], fd)
    part = sref.wavelength_contributions(surf, disp, lam[live], o0, d0)
    ec = np.linalg.norm((chroma[live].astype(np.float64) - fd).reshape(-1, 2, 3), axis=2) / part
    dead = rays[:, 6] == 0
    m = dict(s_med=float(np.median(e)), s_ok=float((e <= 1e-3).mean()), s_tail=float(np.percentile(e, 99.9)),
             l_med=float(np.median(el)), l_tail=float(np.percentile(el, 99.9)), c_med=float(np.median(ec)),
             c_tail=float(np.percentile(ec, 99.9)), finite=bool(np.isfinite(diffs[~dead]).all() and np.isfinite(chroma[~dead]).all()),
             dead_zero=not (_bits(diffs[dead]).any() or _bits(chroma[dead]).any()), dead=int(dead.sum()))
    print(IDS[case], " ".join("%s %.3g" % kv for kv in m.items()))
    _CHECKED[case] = m
    return m


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_spectral_differentials_correct(gpu, oracle_lib, case):
    """Screen tangents: the d-line test's bounds (median <= 1e-5, 99.9 % of the vectors within 1e-3).  Wavelength tangent: against the
    sum of the interfaces' contributions at most 4 x the screen tangents' figures (test_differentials_spectral_cpu has the reasoning)."""
    m = _checked(gpu, oracle_lib, case)
    assert m["finite"] and m["dead_zero"], m
    assert m["s_med"] <= 1e-5 and m["s_ok"] >= 0.999, m
    assert m["c_med"] <= 4 * m["s_med"] and m["c_tail"] <= 4 * m["s_tail"], m


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_wavelength_tangent_ratio_to_its_own_size(gpu, oracle_lib, case):
    """Error relative to the tangent's own size (floor: 1e-3 of the batch's median), median and 99.9th percentile at most 4 x the screen
    tangents' figures on the same rays.  Met because the tangent is traced in f64:
    tests/test_differentials_spectral_cpu.py::test_wavelength_tangent_ratio_to_its_own_size has the reason and the figures."""
    m = _checked(gpu, oracle_lib, case)
    assert m["l_med"] <= 4 * m["s_med"] and m["l_tail"] <= 4 * m["s_tail"], m


@pytest.mark.parametrize("n", SIZES)
def test_d_line_and_flag_identities(gpu, n):
    """all wavelengths 587.5618: the 12 floats are ray_differentials' without wavelengths; chromatic on / off: the same 12 floats; two
    runs are equal; dsx / dsy scale the screen fields only"""
    import torch
    cam = _camera(_params("C2"))
    s = torch.from_numpy(_samples(n, seed=11)).cuda()
    lam = torch.full((n,), float(LAMBDA_D32), device="cuda")
    rays = cam.create_rays(s, wavelengths=lam, ray_index_base=5)["rays"]
    plain = cam.ray_differentials(s, rays, ray_index_base=5)
    d12 = cam.ray_differentials(s, rays, ray_index_base=5, wavelengths=lam)
    d18, ch = cam.ray_differentials(s, rays, ray_index_base=5, wavelengths=lam, chromatic=True)
    assert torch.equal(plain.view(torch.int32), d12.view(torch.int32))
    assert torch.equal(d12.view(torch.int32), d18.view(torch.int32))
    lam2 = torch.from_numpy(np.resize(WAVES, n)).cuda()
    rays2 = cam.create_rays(s, wavelengths=lam2, ray_index_base=5)["rays"]
    a12 = cam.ray_differentials(s, rays2, ray_index_base=5, wavelengths=lam2)
    a18, ach = cam.ray_differentials(s, rays2, ray_index_base=5, wavelengths=lam2, chromatic=True)
    b18, bch = cam.ray_differentials(s, rays2, ray_index_base=5, wavelengths=lam2, chromatic=True)
    assert torch.equal(a12.view(torch.int32), a18.view(torch.int32))
    assert torch.equal(a18.view(torch.int32), b18.view(torch.int32)) and torch.equal(ach.view(torch.int32), bch.view(torch.int32))
    c18, cch = cam.ray_differentials(s, rays2, dsx=0.5, dsy=-0.25, ray_index_base=5, wavelengths=lam2, chromatic=True)
    assert torch.equal(cch.view(torch.int32), ach.view(torch.int32))
    a, c = a18.cpu().numpy(), c18.cpu().numpy()
    live = rays2[:, 6].cpu().numpy() != 0
    assert np.array_equal(c[live][:, np.r_[0:3, 6:9]], (a[live][:, np.r_[0:3, 6:9]] * F32(0.5)).astype(F32))
    assert np.array_equal(c[live][:, np.r_[3:6, 9:12]], (a[live][:, np.r_[3:6, 9:12]] * F32(-0.25)).astype(F32))
    if n >= 4096:
        assert not torch.equal(a12.view(torch.int32), d12.view(torch.int32))   # the wavelengths changed something
    cam.close()


@pytest.mark.parametrize("cfg,V", [("C2", None), ("C5", None), ("C3", 50.0)])
def test_mode_independent_and_split_launches(gpu, cfg, V):
    """STRICT and FAST cameras agree bit for bit wherever their records' tries agree; split launches with ray_index_base equal one"""
    import torch
    p = _params(cfg)
    s = _samples(BIG, seed=13)
    lam = np.random.RandomState(4).uniform(400, 700, BIG).astype(F32)
    a, b = _camera(p, PRECISION_STRICT, _abbe(p, V)), _camera(p, PRECISION_FAST, _abbe(p, V))
    ra, da, ca = _run(a, s, lam, base=1000)
    rb, db, cb = _run(b, s, lam, base=1000)
    same = (_bits(ra[:, 7]) == _bits(rb[:, 7])) & (ra[:, 6] == rb[:, 6])
    assert same.mean() >= 0.9999
    assert np.array_equal(_bits(da[same]), _bits(db[same])) and np.array_equal(_bits(ca[same]), _bits(cb[same]))
    ts, tl, tr = torch.from_numpy(s).cuda(), torch.from_numpy(lam).cuda(), torch.from_numpy(ra).cuda()
    parts_d, parts_c = [], []
    cut = [0, 1, 64, 5000 + 37, BIG]
    for lo, hi in zip(cut[:-1], cut[1:]):
        d, c = a.ray_differentials(ts[lo:hi].contiguous(), tr[lo:hi].contiguous(), ray_index_base=1000 + lo,
                                   wavelengths=tl[lo:hi].contiguous(), chromatic=True)
        parts_d.append(d)
        parts_c.append(c)
    assert np.array_equal(_bits(torch.cat(parts_d).cpu().numpy()), _bits(da))
    assert np.array_equal(_bits(torch.cat(parts_c).cpu().numpy()), _bits(ca))
    a.close()
    b.close()


@pytest.mark.parametrize("over", [{}, dict(useDof=False), dict(opticalVignettingDistance=5.0)], ids=["C1", "C1-noDOF", "C1-vignet"])
def test_thin_lens_ignores_the_wavelength(gpu, over):
    import torch
    cam = _camera(_params("C1", **over))
    n = 4096 + 65
    s = torch.from_numpy(_samples(n, seed=19)).cuda()
    lam = torch.from_numpy(np.random.RandomState(8).uniform(360, 830, n).astype(F32)).cuda()
    rays = cam.create_rays(s, wavelengths=lam)["rays"]
    plain = cam.ray_differentials(s, rays)
    d, c = cam.ray_differentials(s, rays, wavelengths=lam, chromatic=True)
    assert torch.equal(plain.view(torch.int32), d.view(torch.int32))
    assert not c.view(torch.int32).any()
    assert plain.abs().sum() > 0
    cam.close()


@pytest.mark.parametrize("cfg", ["C2", "C5", "C1"])
def test_zeros(gpu, cfg):
    """weight-0 rows, the forward call's rejected rows and rows given a bad wavelength HERE although their record is live: +0.0 in every
    float; their live neighbours in the same wave are untouched; a wave that is wholly dead"""
    import torch
    cam = _camera(_params(cfg))
    n = 4096 + 63
    s_np = _samples(n, seed=23)
    lam_np = np.random.RandomState(6).uniform(400, 700, n).astype(F32)
    fwd = lam_np.copy()
    fwd_bad = np.arange(len(BAD)) * 9 + 130          # rejected by the forward call (flags 0x80), mixed into waves 2 and 3
    fwd[fwd_bad] = BAD
    s, tf = torch.from_numpy(s_np).cuda(), torch.from_numpy(fwd).cuda()
    rays = cam.create_rays(s, wavelengths=tf)["rays"]
    r = rays.cpu().numpy()
    assert (r[fwd_bad, 7].view(np.uint32) == 0x80).all()
    ref_d, ref_c = [x.cpu().numpy() for x in cam.ray_differentials(s, rays, wavelengths=tf, chromatic=True)]
    assert not _bits(ref_d[fwd_bad]).any() and not _bits(ref_c[fwd_bad]).any()
    dead = r[:, 6] == 0
    assert not _bits(ref_d[dead]).any() and not _bits(ref_c[dead]).any()
    # bad wavelengths here on live records: one in each lane position of BAD within wave 5, and the whole of wave 7
    live_rows = np.nonzero(~dead)[0]
    here = lam_np.copy()
    mixed = live_rows[(live_rows >= 320) & (live_rows < 384)][:len(BAD)]
    assert len(mixed) == len(BAD)
    here[mixed] = BAD
    here[448:512] = np.resize(BAD, 64)
    here[fwd_bad] = fwd[fwd_bad]
    got_d, got_c = [x.cpu().numpy() for x in cam.ray_differentials(s, rays, wavelengths=torch.from_numpy(here).cuda(), chromatic=True)]
    zero = np.zeros(n, bool)
    zero[mixed] = True
    zero[448:512] = True
    assert (~dead[448:512]).any() or cfg == "C5"
    assert not _bits(got_d[zero]).any() and not _bits(got_c[zero]).any()
    assert np.array_equal(_bits(got_d[~zero]), _bits(ref_d[~zero])) and np.array_equal(_bits(got_c[~zero]), _bits(ref_c[~zero]))
    assert (_bits(ref_d[mixed]) != 0).any()
    # a wave whose records are all dead: every weight set to 0
    r2 = rays.clone()
    r2[64:128, 6] = 0.0
    d2, c2 = [x.cpu().numpy() for x in cam.ray_differentials(s, r2, wavelengths=tf, chromatic=True)]
    assert not _bits(d2[64:128]).any() and not _bits(c2[64:128]).any()
    keep = np.r_[0:64, 128:n]
    assert np.array_equal(_bits(d2[keep]), _bits(ref_d[keep])) and np.array_equal(_bits(c2[keep]), _bits(ref_c[keep]))
    cam.close()


def test_lens_model_none_gives_zeros(gpu):
    import torch
    cam = _camera(_params("C2"))
    s = torch.from_numpy(_samples(4096)).cuda()
    lam = torch.full((4096,), 500.0, device="cuda")
    rays = cam.create_rays(s, wavelengths=lam)["rays"]
    cam.update(**_params("C2", lensModel=2))
    out = torch.full((4096, 12), 7.0, device="cuda")
    d, c = cam.ray_differentials(s, rays, out=out, wavelengths=lam, chromatic=True)
    torch.cuda.synchronize()
    assert not d.view(torch.int32).any() and not c.view(torch.int32).any()
    cam.close()


def test_abbe_override_is_honoured_from_the_next_call(gpu):
    import torch
    p = _params("C3")
    cam = _camera(p)
    n = 4096
    s = torch.from_numpy(_samples(n, seed=29)).cuda()
    lam = torch.full((n,), 450.0, device="cuda")
    rays = cam.create_rays(s, wavelengths=lam)["rays"]
    d0, c0 = cam.ray_differentials(s, rays, wavelengths=lam, chromatic=True)
    assert torch.equal(d0.view(torch.int32), cam.ray_differentials(s, rays).view(torch.int32))   # no V-numbers: the d-line's
    assert not (c0.view(torch.int32) & 0x7FFFFFFF).any()
    cam.set_abbe_numbers(_abbe(p, 50.0))
    d1, c1 = cam.ray_differentials(s, rays, wavelengths=lam, chromatic=True)
    assert not torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and bool(c1.abs().sum() > 0)
    cam.close()


def test_error_codes(gpu):
    import torch
    lib = gpu
    OK, INVALID, NOT_UPDATED = 0, _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT"), _capi.STATUS_NAMES.index("ZOIC_ERR_NOT_UPDATED")
    cam = ZoicCamera(device=0)
    s = torch.zeros((64, 4), device="cuda")
    r = torch.zeros((64, 8), device="cuda")
    o = torch.zeros((65, 12), device="cuda")
    c = torch.zeros((65, 6), device="cuda")
    w = torch.full((65,), 500.0, device="cuda")
    st = C.c_void_p(0)
    f = lib.zoic_ray_differentials_spectral_device
    S, R, O, Cc, W = s.data_ptr(), r.data_ptr(), o.data_ptr(), c.data_ptr(), w.data_ptr()
    assert f(cam._h, 64, S, W, None, 0, R, 1.0, 1.0, O, Cc, st) == NOT_UPDATED
    cam.update(**_params("C2"))
    assert f(cam._h, 0, None, None, None, 0, None, 1.0, 1.0, None, None, st) == OK
    assert f(cam._h, 64, S, W, None, 0, R, 1.0, 1.0, O, None, st) == OK
    assert f(cam._h, 64, S, W + 4, None, 0, R, 1.0, 1.0, O, Cc + 8, st) == OK
    assert f(None, 64, S, W, None, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, None, W, None, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S + 4, W, None, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, None, None, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, W + 2, None, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, S + 8, 0, R, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, None, 0, None, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, None, 0, R + 4, 1.0, 1.0, O, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, None, 0, R, 1.0, 1.0, None, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, None, 0, R, 1.0, 1.0, O + 4, Cc, st) == INVALID
    assert f(cam._h, 64, S, W, None, 0, R, 1.0, 1.0, O, Cc + 4, st) == INVALID
    torch.cuda.synchronize()
    w64 = w[:64].contiguous()
    with pytest.raises(ValueError):
        cam.ray_differentials(s, r, chromatic=True)
    with pytest.raises(ValueError):
        cam.ray_differentials(s, r, wavelengths=w64.double())
    with pytest.raises(ValueError):
        cam.ray_differentials(s, r, wavelengths=w)                # 65 for 64 rays
    with pytest.raises(ValueError):
        cam.ray_differentials(s, r, wavelengths=w64.cpu())
    with pytest.raises(TypeError):
        cam.ray_differentials(s, r, wavelengths=np.full(64, 500.0, F32))
    assert tuple(cam.ray_differentials(s, r, wavelengths=w64).shape) == (64, 12)
    cam.close()


def test_host_equals_device(gpu, oracle_lib):
    """The host build of csrc/differentials_spectral.hpp from the same starts against the kernel.  diff_rsqrt / diff_sqrt / diff_rcp are
    1-ulp instructions on the device, so not bitwise: the screen tangents within the d-line test's figures for this arithmetic
    (median <= 1e-5, 99.9 % within 1e-3: device and host each meet them against f64), the wavelength tangent within the same bounds
    measured against the sum of its contributions."""
    p = _params("C2")
    cam = _camera(p)
    disp = cam.dispersion()
    n = 4096
    s = _samples(n, seed=31)
    lam = np.resize(WAVES, n)
    states = ray_rng_states(n, seed=1)
    rays, diffs, chroma = _run(cam, s, lam)
    cam.close()
    live = np.nonzero(rays[:, 6] != 0)[0]
    tries = ((rays[live, 7].view(np.uint32) >> 1) & 31).astype(np.int64)
    oc = _oracle(oracle_lib, p)
    o0, d0 = dref.kolb_start(oc, p, s[live], tries, states[live], oracle_lib)
    surf = dref.surfaces(oc.lens_table())
    hs = F32(F32(p["sensorWidth"]) * F32(0.5))
    out, ch, prim = run_driver(host_drivers.differentials_spectral(), 2, surf, disp, hs, lam[live], o0, d0)
    assert np.allclose(prim, rays[live, 0:6], rtol=1e-5, atol=1e-5)
    e = dref.rel_err(diffs[live], out)
    part = sref.wavelength_contributions(surf, disp, lam[live], o0, d0)
    ec = np.linalg.norm((chroma[live].astype(np.float64) - ch).reshape(-1, 2, 3), axis=2) / part
    print("host vs device: screen %.2e / %.2e, wavelength %.2e / %.2e" %
          (float(np.median(e)), float(e.max()), float(np.median(ec)), float(ec.max())))
    assert np.median(e) <= 1e-5 and (e <= 1e-3).mean() >= 0.999
    assert np.median(ec) <= 1e-5 and (ec <= 1e-3).mean() >= 0.999

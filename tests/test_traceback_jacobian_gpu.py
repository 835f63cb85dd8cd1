"""The trace-back Jacobian on the MI355X (zoic_trace_back_jacobian_device and its spectral form): the batch kernels give the host
calls' bits -- Ps, flags and all twelve entries of J -- deterministically and whatever the batch size; the records a camera writes are
taken back on the device buffer they were written to, into the caller's tensors, without touching a counter; J composed with the
forward ray differentials of the same samples is the identity as nearly as the f32 finite-difference Jacobian makes it; bad
pointers are refused before any launch.

Frame 64 x 36 x 2 (4 608 rays)."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import traceback_cases as tc
import traceback_jacobian_ref as jr
from device_cases import bits as _bits, records as _records
from traceback_jacobian_ref import H, N, SPP, W, residual as _residual
from traceback_ref import TraceBack

SLAB = 2048 * 256   # one grid of the kernels (kPassGridCap x kPassBlock, device_pass.hpp): larger batches are walked slab by slab
EDGE_ROWS = np.array([[0, 0, -1, 0, 0, -1], [0, 0, -1e30, 0, 0, -1e-30], [1e30, 0, -1, 0, 0, -1], [0, 0, -1, 1e30, 0, -1e-30],
                      [0, 0, 0, 0, 0, -1], [-0.0, -0.0, -0.0, -0.0, -0.0, -1], [0, 0, -1, 1, 0, -1e-38], [1e-30, 1e-30, -1e-30, 1e-30, 0, -1e-30]],
                     np.float32)
# the yardstick's step per configuration: the one tests/test_traceback_jacobian_cpu.py finds best for it
YARDSTICK_H = {"C1": 2.0 ** -8, "C2": 2.0 ** -9, "C3": 2.0 ** -8}


def _camera(cfg, precision=PRECISION_STRICT, **over):
    p = dict(camera_params(cfg), **over)
    cam = ZoicCamera(device=0)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    cam.set_precision(precision)
    cam.update(**p)
    return cam, p


def _ray_set(cam, p):
    """the frame's records (whatever their weight), the refusal families, the non-finite rays, random lines and the edge rows"""
    fwd = cam.create_rays(synthetic_samples(N, W, H, SPP), rng_states=ray_rng_states(N))
    rec = np.ascontiguousarray(fwd["rays"]).view(np.float32).reshape(-1, 8)
    info = cam.info()
    sets = [rec, _records(*tc.non_finite_rays()), _records(*tc.random_lines(info, 1024)), _records(EDGE_ROWS[:, :3], EDGE_ROWS[:, 3:])]
    if p["lensModel"] == _capi.RAYTRACED:
        live = np.flatnonzero(fwd["weight"] > 0)[::16]
        sets += [_records(o, d) for o, d in tc.rejection_families(info, rec[live, 0:3], rec[live, 3:6]).values()]
    return np.ascontiguousarray(np.concatenate(sets), dtype=np.float32), int((fwd["weight"] > 0).sum())


def _check_against_host(cam, p, rays, lam, n_live, tiled):
    import torch
    scr, fl, jac = cam.trace_back_jacobian(rays, wavelengths=lam)
    hs, hf, hj = jr.host_jacobian(cam, rays[:, 0:3], rays[:, 3:6], lam)
    assert jac.shape == (len(rays), 2, 6) and jac.dtype == np.float32
    assert np.array_equal(_bits(scr), _bits(hs))
    assert np.array_equal(fl.astype(np.uint32), hf)
    assert np.array_equal(_bits(jac), _bits(hj))
    traced = (hf & 1) == 1
    assert traced.sum() > 0.9 * n_live * (1.0 if lam is None else 0.7)
    assert (_bits(jac[~traced]) == 0).all()
    assert len(set(tc.reason(hf[~traced]).tolist())) >= (3 if p["lensModel"] == _capi.RAYTRACED else 2)
    # and the existing trace-back kernel's Ps and flags
    s0, f0 = cam.trace_back(rays, wavelengths=lam)
    assert np.array_equal(_bits(s0), _bits(scr)) and np.array_equal(f0, fl)
    # twice: the same bits; prefixes of the same rays
    scr2, fl2, jac2 = cam.trace_back_jacobian(rays, wavelengths=lam)
    assert np.array_equal(_bits(scr2), _bits(scr)) and np.array_equal(fl2, fl) and np.array_equal(_bits(jac2), _bits(jac))
    for k in (1, 63, 64, 65, 777):
        s, f, j = cam.trace_back_jacobian(rays[:k], wavelengths=None if lam is None else lam[:k])
        assert np.array_equal(_bits(s), _bits(scr[:k])) and np.array_equal(f, fl[:k]) and np.array_equal(_bits(j), _bits(jac[:k])), k
    if tiled:   # more than one slab
        reps = SLAB // len(rays) + 2
        big = torch.from_numpy(np.tile(rays, (reps, 1))).to("cuda:0")
        bl = None if lam is None else torch.from_numpy(np.tile(lam, reps)).to("cuda:0")
        s, f, j = cam.trace_back_jacobian(big, wavelengths=bl)
        torch.cuda.synchronize()
        assert big.shape[0] > SLAB
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(np.tile(scr, (reps, 1))))
        assert np.array_equal(f.cpu().numpy(), np.tile(fl, reps))
        assert np.array_equal(_bits(j.cpu().numpy()), _bits(np.tile(jac, (reps, 1, 1))))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_kernel_equals_host_bitwise(gpu, oracle_lib, cfg):
    cam, p = _camera(cfg)
    rays, n_live = _ray_set(cam, p)
    _check_against_host(cam, p, rays, None, n_live, tiled=cfg == "C3")
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_spectral_kernel_equals_host_bitwise(gpu, oracle_lib, cfg):
    cam, p = _camera(cfg)
    bs.set_dispersion(cam, cfg)
    rays, n_live = _ray_set(cam, p)
    lam = np.linspace(400.0, 700.0, len(rays)).astype(np.float32)
    lam[::7] = np.float32(587.5618)
    lam[5] = np.float32(900.0)   # one invalid wavelength
    _check_against_host(cam, p, rays, lam, n_live, tiled=cfg == "C2")
    scr, fl, jac = cam.trace_back_jacobian(rays[:64], wavelengths=lam[:64])
    assert tc.reason(fl[5]) == bs.TB_WAVELENGTH and (_bits(jac[5]) == 0).all() and (_bits(scr[5]) == 0).all()
    cam.close()


@pytest.mark.gpu
def test_in_place_outputs_and_counters(gpu, oracle_lib):
    import torch
    cam, p = _camera("C2")
    smp = torch.from_numpy(synthetic_samples(N, W, H, SPP)).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(N).view(np.int32)).to("cuda:0")
    before = cam.counters()
    fwd = cam.create_rays(smp, rng_states=st)
    after = cam.counters()
    scr, fl, jac = cam.trace_back_jacobian(fwd)   # the dict create_rays returned: its buffer is read in place, on the same stream
    torch.cuda.synchronize()
    assert cam.counters() == after and after != before
    rec = fwd["rays"].cpu().numpy()
    hs, hf, hj = jr.host_jacobian(cam, rec[:, 0:3], rec[:, 3:6])
    assert np.array_equal(_bits(scr.cpu().numpy()), _bits(hs)) and np.array_equal(_bits(jac.cpu().numpy()), _bits(hj))
    assert (fl & 1).sum().item() > N // 2
    out = torch.full((N, 2), 7.0, dtype=torch.float32, device="cuda:0")
    flags = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    jacobian = torch.full((N, 2, 6), 7.0, dtype=torch.float32, device="cuda:0")
    o2, f2, j2 = cam.trace_back_jacobian(fwd["rays"], out=out, flags=flags, jacobian=jacobian)
    torch.cuda.synchronize()
    assert o2.data_ptr() == out.data_ptr() and f2.data_ptr() == flags.data_ptr() and j2.data_ptr() == jacobian.data_ptr()
    assert torch.equal(out, scr) and torch.equal(flags, fl) and np.array_equal(_bits(jacobian.cpu().numpy()), _bits(jac.cpu().numpy()))
    assert cam.counters() == after
    # numpy records in, numpy out
    s3, f3, j3 = cam.trace_back_jacobian(np.ascontiguousarray(rec).view(_capi.RAY_DTYPE).reshape(-1))
    assert np.array_equal(s3, scr.cpu().numpy()) and np.array_equal(f3, fl.cpu().numpy()) and np.array_equal(_bits(j3), _bits(hj))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_round_trip_against_the_forward_differentials(gpu, oracle_lib, name):
    """FAST camera.  T = [dOdx dOdy; dDdx dDdy] of the forward differentials (dsx = dsy = 1): with the lens point held fixed every
    member of that ray family traces back to its own sample, so J T = I.  The residual |J T - I|_max of the kernel's J is held to
    1.5 x the residual of the f32 finite-difference Jacobian (median and p99, on the same rays): both carry the forward
    differentials' own error, which neither can go below.

    The yardstick is taken on 512 rays by the host call, with the step of the CPU test.  A record's origin lies on the front element's
    cap, where the neighbours origin - h s_o e_z are refused (kTbAway); so the finite differences are taken at o' = o + k dir, one front
    housing radius out on the same line, and brought back: Ps(o + k dir, dir) = Ps(o, dir) gives J_o(o) = J_o(o') and
    J_d(o) = J_d(o') + k J_o(o')."""
    import torch
    cam, p = _camera(name, PRECISION_FAST)
    info = cam.info()
    smp = torch.from_numpy(synthetic_samples(N, W, H, SPP)).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(N).view(np.int32)).to("cuda:0")
    fwd = cam.create_rays(smp, rng_states=st)
    diffs = cam.ray_differentials(smp, fwd, rng_states=st)
    scr, fl, jac = cam.trace_back_jacobian(fwd)
    torch.cuda.synchronize()
    rec, diffs, jac, fl = fwd["rays"].cpu().numpy(), diffs.cpu().numpy().astype(np.float64), jac.cpu().numpy(), fl.cpu().numpy()
    T = np.concatenate([np.stack([diffs[:, 0:3], diffs[:, 3:6]], 2), np.stack([diffs[:, 6:9], diffs[:, 9:12]], 2)], 1)   # (n,6,2)
    Tb = TraceBack(info, p)
    o, d = rec[:, 0:3], rec[:, 3:6]
    ref = Tb.trace(o, d)
    keep = (rec[:, 6] > 0) & ref["traced"] & ~Tb.edge(ref) & ((fl & 1) == 1) & (np.abs(T).max((1, 2)) > 0)
    assert keep.sum() > 0.5 * (rec[:, 6] > 0).sum()
    # the yardstick on 512 rays
    pick = np.flatnonzero(keep)[:: max(1, keep.sum() // 512)][:512]
    s = jr.scales(info, p)
    k = s[0] / np.linalg.norm(d[pick].astype(np.float64), axis=1)   # one scale out along the ray
    o1 = (o[pick].astype(np.float64) + k[:, None] * d[pick].astype(np.float64)).astype(np.float32)
    k = ((o1.astype(np.float64) - o[pick]) * d[pick]).sum(1) / (d[pick].astype(np.float64) ** 2).sum(1)   # the move actually made
    Y, ok = jr.yardstick(cam, o1, d[pick], s, YARDSTICK_H[name])
    Y[:, :, 3:] += k[:, None, None] * Y[:, :, :3]
    pick, Y = pick[ok], Y[ok]
    assert len(pick) >= 384, len(pick)
    rj = _residual(jac[pick].astype(np.float64), T[pick])
    ry = _residual(Y, T[pick])
    print("%s: %d rays; |J T - I| median %.3g p99 %.3g; finite differences median %.3g p99 %.3g; all %d kept rays: median %.3g p99 %.3g"
          % (name, len(pick), np.median(rj), np.percentile(rj, 99), np.median(ry), np.percentile(ry, 99), keep.sum(),
             np.median(_residual(jac[keep].astype(np.float64), T[keep])), np.percentile(_residual(jac[keep].astype(np.float64), T[keep]), 99)))
    assert np.median(rj) <= 1.5 * np.median(ry), (np.median(rj), np.median(ry))
    assert np.percentile(rj, 99) <= 1.5 * np.percentile(ry, 99), (np.percentile(rj, 99), np.percentile(ry, 99))
    cam.close()


@pytest.mark.gpu
def test_argument_errors(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C2")
    n = 1024
    rays = cam.create_rays(torch.from_numpy(synthetic_samples(n, 32, 32, 1)).to("cuda:0"))["rays"]
    lam = torch.full((n + 1,), 550.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda:0")
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    jac = torch.full((n + 1, 2, 6), 7.0, dtype=torch.float32, device="cuda:0")
    host = np.zeros((n, 12), np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    R, L, O, F, J = rays.data_ptr(), lam.data_ptr(), out.data_ptr(), flags.data_ptr(), jac.data_ptr()
    d, s = lib.zoic_trace_back_jacobian_device, lib.zoic_trace_back_jacobian_spectral_device
    before = cam.counters()
    assert d(cam._h, n, None, O, F, J, st) == 1
    assert d(cam._h, n, R, None, F, J, st) == 1
    assert d(cam._h, n, R, O, F, None, st) == 1
    assert d(cam._h, n, R, O, F, J + 4, st) == 1                    # d_jacobian misaligned by 4 bytes
    assert d(cam._h, n, R, O, F, host.ctypes.data, st) == 1         # a host pointer
    assert d(cam._h, n, host.ctypes.data, O, F, J, st) == 1
    assert d(cam._h, n - 1, R + 8, O, F, J, st) == 1
    assert d(cam._h, n - 1, R, O + 4, F, J, st) == 1
    assert d(cam._h, n - 1, R, O, F + 2, J, st) == 1
    assert d(cam._h, 0, None, None, None, None, st) == 0            # n = 0: no-op
    assert s(cam._h, n, R, None, O, F, J, st) == 1                  # NULL d_wavelengths
    assert s(cam._h, n, R, L + 2, O, F, J, st) == 1                 # misaligned d_wavelengths
    assert s(cam._h, n, R, L, O, F, J + 4, st) == 1
    assert s(cam._h, n, R, L, O, F, None, st) == 1
    assert s(cam._h, n, None, L, O, F, J, st) == 1
    assert s(cam._h, n, R, L, None, F, J, st) == 1
    assert s(cam._h, 0, None, None, None, None, None, st) == 0
    fresh = ZoicCamera(device=0)
    assert d(fresh._h, n, R, O, None, J, st) == 9                   # NOT_UPDATED
    assert s(fresh._h, n, R, L, O, None, J, st) == 9
    fresh.close()
    torch.cuda.synchronize()
    # nothing was launched: the outputs are untouched
    assert (out == 7.0).all().item() and (flags == -1).all().item() and (jac == 7.0).all().item() and cam.counters() == before
    assert d(cam._h, n, R, O, None, J, st) == 0                     # flags may be NULL
    torch.cuda.synchronize()
    assert (flags == -1).all().item() and not (jac[:n] == 7.0).all().item() and (jac[n] == 7.0).all().item()
    cam.close()
    host_cam = tc.update(ZoicCamera(device=-1), tc.params_of("C2"))
    assert d(host_cam._h, n, R, O, F, J, st) == 11                  # a tables-only camera: NO_DEVICE
    assert s(host_cam._h, n, R, L, O, F, J, st) == 11
    host_cam.close()

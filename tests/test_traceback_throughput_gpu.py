"""Trace-back transmittance on the MI355X (zoic_trace_back_transmittance_device, zoic_splat_transmittance_device and their _spectral
forms): the kernels give the host twin's bits -- T, screen sample and flag word -- whatever the batch size, bare and coated, at the
d-line and at a wavelength per ray; screen and flags are the trace-back call's; the splat side is the ray side on the rays of the
splat records; the backward T of a frame's spectral records is the forward call's to the CPU test's bound; the calls touch no counter
and no retry stream, refuse bad arguments before any launch and follow updates and setters.

Host twin: the library's own host calls (zoic_trace_back_ray_transmittance, zoic_splat_point_transmittance: the same header compiled
for the host), which tests/test_traceback_throughput_cpu.py holds against an f64 restatement."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi, pupil_bounds_records
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr
import transmittance_ref as tref
from device_cases import bits_f32 as _bits, records as _records

F32 = np.float32
W, H, SPP = 96, 54, 1      # 5 184 forward records
G = 16
SHAPES = ((1, 1), (3, 5), (5, 64), (2, 257), (174763, 3))      # tests/test_splats_gpu.py's, the grid-stride shape included
assert SHAPES[-1][0] * SHAPES[-1][1] == mc.GRID_PLUS_ONE
CAMERAS = {"C3-strict": ("C3", PRECISION_STRICT), "C3-fast": ("C3", PRECISION_FAST), "C2": ("C2", PRECISION_STRICT)}


def _camera(name, precision=PRECISION_STRICT):
    p = tc.params_of(name)
    cam = ZoicCamera(device=0)
    cam.set_precision(precision)
    tc.update(cam, p)
    return bs.set_dispersion(cam, name), p


def _films(cam):
    return tref.films_where_media_differ(cam.dispersion())


def _batch(cam, p):
    """(rays (m,8) f32, wavelengths (m,) f32): the forward records of a small frame, whatever their weight, then the rays every reason
    refuses; valid and invalid wavelengths interleaved"""
    n = W * H * SPP
    fwd = cam.create_rays(synthetic_samples(n, W, H, SPP), rng_states=ray_rng_states(n))
    rec = np.ascontiguousarray(fwd["rays"]).view(F32).reshape(-1, 8)
    info = cam.info()
    live = np.flatnonzero(fwd["weight"] > 0)[::8]
    sets = [rec, _records(*tc.non_finite_rays()), _records(*tc.random_lines(info, 2048))]
    sets += [_records(o, d) for o, d in tc.rejection_families(info, rec[live, 0:3], rec[live, 3:6]).values()]
    rays = np.ascontiguousarray(np.concatenate(sets), F32)
    return rays, bs.mixed_wavelengths(len(rays))


def _same(got, want):
    """(T, screen, flags) of a device call against (ps, flags, T) of the host twin, bit for bit"""
    T, scr, fl = (np.asarray(a) for a in got)
    ps, hf, hT = want
    return np.array_equal(_bits(T), _bits(hT)) and np.array_equal(scr.view(np.uint32), ps.view(np.uint32)) and \
        np.array_equal(fl.astype(np.uint32), hf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CAMERAS))
def test_kernel_equals_host_twin_bitwise(gpu, name):
    import torch
    cfg, precision = CAMERAS[name]
    cam, p = _camera(cfg, precision)
    rays, lam = _batch(cam, p)
    films = _films(cam)
    big = mc.GRID_PLUS_ONE
    reps = -(-big // len(rays))
    dev = torch.device("cuda", 0)
    big_rays = torch.from_numpy(np.tile(rays, (reps, 1))[:big].copy()).to(dev)
    big_lam = torch.from_numpy(np.tile(lam, reps)[:big].copy()).to(dev)
    pick = np.arange(0, big, 128)
    half = big // 2 + 1      # odd: the second launch's buffers start off the 16-byte grid of their element sizes where they may
    for coated in (False, True):
        tr.coat(cam, films if coated else None)
        for w in (None, lam):
            host = tr.lib_throughput(cam, rays[:, 0:3], rays[:, 3:6], w)
            got = cam.trace_back_transmittance(rays, wavelengths=w)
            assert _same(got, host), (name, coated, w is not None)
            hf = host[1]
            reasons = set(tc.reason(hf[(hf & 1) == 0]).tolist())
            assert (hf & 1).sum() >= 2048 and reasons >= ({1, 2, 3, 4, 5} | ({bs.TB_WAVELENGTH} if w is not None else set())), reasons
            # screen and flags are the trace-back call's
            scr, fl = cam.trace_back(rays, wavelengths=w)
            assert np.array_equal(scr.view(np.uint32), got[1].view(np.uint32)) and np.array_equal(fl, got[2])
            for k in mc.PREFIXES:
                part = cam.trace_back_transmittance(rays[:k], wavelengths=None if w is None else w[:k])
                assert _same(part, tuple(a[:k] for a in host)), (name, coated, k)
            # one grid and one ray more: a strided sample against the host twin, every ray against a second launch split in two
            bw = None if w is None else big_lam
            T, s, f = cam.trace_back_transmittance(big_rays, wavelengths=bw)
            a = cam.trace_back_transmittance(big_rays[:half], wavelengths=None if w is None else bw[:half])
            b = cam.trace_back_transmittance(big_rays[half:], wavelengths=None if w is None else bw[half:])
            torch.cuda.synchronize()
            for whole, x, y in zip((T, s, f), a, b):
                assert torch.equal(whole.view(torch.int32), torch.cat([x, y]).view(torch.int32)), (name, coated)
            src = pick % len(rays)
            assert _same((T.cpu().numpy()[pick], s.cpu().numpy()[pick], f.cpu().numpy()[pick]), tuple(a[src] for a in host))
    cam.close()


@pytest.mark.gpu
def test_outputs_may_be_null_and_the_records_are_read_in_place(gpu):
    """d_screen / d_flags NULL: the same T; and the rays are the buffer a forward call wrote on the same stream"""
    import torch
    lib = _capi.load()
    cam, p = _camera("C3")
    tr.coat(cam, _films(cam))
    n = 4097
    smp = torch.from_numpy(synthetic_samples(n, 241, 17, 1)).to("cuda:0")
    lam = torch.from_numpy(bs.mixed_wavelengths(n)).to("cuda:0")
    want_rays = cam.create_rays(smp, wavelengths=lam)["rays"].clone()
    want = cam.trace_back_transmittance(want_rays, wavelengths=lam)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fwd = cam.create_rays(smp, wavelengths=lam, out=dict(rays=rays), stream=side.cuda_stream)
    got = cam.trace_back_transmittance(fwd, wavelengths=lam, stream=side.cuda_stream)      # the dict: its buffer is read in place
    side.synchronize()
    assert torch.equal(rays, want_rays)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (want[0] > 0).sum().item() > n // 4
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for spectral in (False, True):
        ref = cam.trace_back_transmittance(rays, wavelengths=lam if spectral else None)
        for with_screen, with_flags in ((False, False), (True, False), (False, True)):
            T = torch.full((n,), 7.0, dtype=torch.float32, device="cuda:0")
            scr = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda:0")
            fl = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
            tail = (T.data_ptr(), scr.data_ptr() if with_screen else None, fl.data_ptr() if with_flags else None, st)
            if spectral:
                rc = lib.zoic_trace_back_transmittance_spectral_device(cam._h, n, rays.data_ptr(), lam.data_ptr(), *tail)
            else:
                rc = lib.zoic_trace_back_transmittance_device(cam._h, n, rays.data_ptr(), *tail)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(T.view(torch.int32), ref[0].view(torch.int32))
            assert torch.equal(scr.view(torch.int32), ref[1].view(torch.int32)) if with_screen else (scr == 7.0).all().item()
            assert torch.equal(fl, ref[2]) if with_flags else (fl == -1).all().item()
    cam.close()


def _u(n, m):
    u = np.random.default_rng(1000 * n + m).random((n, m, 2)).astype(F32)
    u[0, 0] = (0.5, 0.5)
    if m > 2:
        u[n // 2, 1] = (np.nan, 0.5)     # a NaN aim: refused by the trace
        u[n - 1, 2] = (-1.0, 2.0)        # outside the unit square: the box's edge
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C3", "C1", "C3-f8"])
def test_splat_side_is_the_ray_side_on_the_splat_rays(gpu, name):
    import torch
    p = pc.params_of(name)
    cam = tc.update(ZoicCamera(device=0), p)
    cfg = pc.CAMERAS[name][0]
    if cfg in tc.KOLB:
        bs.set_dispersion(cam, cfg)
        tr.coat(cam, _films(cam))
    dev = torch.device("cuda", 0)
    z = F32(cam.pupil_square()[0])
    side = torch.cuda.Stream(dev)
    for n, m in SHAPES if name == "C3" else SHAPES[:-1]:
        pts_h, u_h = pc.batch(p, n), _u(n, m)
        lam_h = np.resize(pc.wavelengths(10), n).astype(F32)
        for w in (None, lam_h):
            with torch.cuda.stream(side):
                P, Uu = torch.from_numpy(pts_h).to(dev), torch.from_numpy(u_h).to(dev)
                L = None if w is None else torch.from_numpy(w).to(dev)
                bounds = cam.pupil_bounds(P, G)          # the d-line boxes, written on this stream: an invalid wavelength reaches the trace
                T = cam.splat_transmittance(P, bounds, Uu, L)
                rec = cam.splat_points(P, bounds, Uu, L)
                # the rays of the records: origin P, dir P - A
                A = torch.cat([rec[:, :, 2:4], torch.full((n, m, 1), float(z), device=dev)], 2)
                O = P[:, None, :].expand(n, m, 3)
                rays = torch.zeros((n * m, 8), dtype=torch.float32, device=dev)
                rays[:, 0:3] = O.reshape(-1, 3)
                rays[:, 3:6] = (O - A).reshape(-1, 3)
                Tr, _, fr = cam.trace_back_transmittance(rays, wavelengths=None if L is None else L.repeat_interleave(m))
            side.synchronize()
            assert tuple(T.shape) == (n, m) and T.dtype == torch.float32
            flags = rec[:, :, 6].view(torch.int32)
            boxed = flags != _capi.SPLAT_NO_BOX
            assert torch.equal((T > 0), (flags & 1) == 1) and (T.view(torch.int32)[~(T > 0)] == 0).all().item() and (T <= 1).all().item()
            assert torch.equal(T.view(torch.int32)[boxed], Tr.view(torch.int32).reshape(n, m)[boxed]), (name, n, m, w is not None)
            assert torch.equal(flags[boxed], fr.reshape(n, m)[boxed])
            assert (T > 0).any().item()
            if n <= 5:      # and the host twin's bits
                b = pupil_bounds_records(bounds)
                for i in range(n):
                    host = cam.splat_point_transmittance(pts_h[i], b[i:i + 1], u_h[i], None if w is None else w[i])
                    assert np.array_equal(_bits(host), _bits(T[i].cpu().numpy())), (name, n, m, i)
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
def test_reciprocity_on_the_device(gpu, coated):
    """zoic_ray_transmittance_device on a frame's spectral records against this call on the same records: equal within the CPU test's
    asserted bound plus its E_rec, on the rays both trace.  Measured on 32 757 of 32 768 records: 2.98e-7 bare, 4.77e-7 with the film
    (the sum asserted: 2.35e-6)"""
    import torch
    cam, p = _camera("C3")
    tr.coat(cam, _films(cam) if coated else None)
    n = 1 << 15
    smp = torch.from_numpy(synthetic_samples(n, 256, 128, 1)).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(n).view(np.int32)).to("cuda:0")
    lam = torch.from_numpy(np.random.default_rng(2).uniform(400.0, 700.0, n).astype(F32)).to("cuda:0")
    fwd = cam.create_rays(smp, wavelengths=lam, rng_states=st)
    Tf = cam.transmittance(smp, fwd["rays"], wavelengths=lam, rng_states=st)
    Tb, _, fl = cam.trace_back_transmittance(fwd, wavelengths=lam)
    torch.cuda.synchronize()
    both = (Tf > 0) & (Tb > 0)
    diff = (Tf.double() - Tb.double()).abs()[both].max().item()
    print("%s: both trace %d of %d; largest |T_forward - T_backward| %.3g" % ("film" if coated else "bare", both.sum().item(), n, diff))
    assert both.sum().item() >= n // 2
    assert diff <= tr.BOUND + tr.E_REC, diff
    cam.close()


@pytest.mark.gpu
def test_torch_path_counters_and_retry_streams(gpu):
    """a side stream, out= reuse, and nothing else of the camera moves: counters() before equals after, and create_rays with the same
    retry-stream states gives the same records after as before"""
    import torch
    cam, p = _camera("C3")
    nr = 4096
    smp, st = synthetic_samples(nr, 64, 32, 2), ray_rng_states(nr)
    first = cam.create_rays(smp, rng_states=st)["rays"].copy()
    before = cam.counters()
    rays_h, lam_h = _batch(cam, p)
    after_forward = cam.counters()
    n = len(rays_h)
    side = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(side):
        rays, lam = torch.from_numpy(rays_h).to("cuda:0"), torch.from_numpy(lam_h).to("cuda:0")
        T = torch.full((n,), 7.0, dtype=torch.float32, device="cuda:0")
        scr = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda:0")
        fl = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        res = cam.trace_back_transmittance(rays, out=T, screen=scr, flags=fl)
        assert [t.data_ptr() for t in res] == [T.data_ptr(), scr.data_ptr(), fl.data_ptr()]
        spectral = cam.trace_back_transmittance(rays, lam, stream=side.cuda_stream)
    side.synchronize()
    assert cam.counters() == after_forward and after_forward != before
    assert _same((T.cpu().numpy(), scr.cpu().numpy(), fl.cpu().numpy()), tr.lib_throughput(cam, rays_h[:, 0:3], rays_h[:, 3:6]))
    assert _same(tuple(t.cpu().numpy() for t in spectral), tr.lib_throughput(cam, rays_h[:, 0:3], rays_h[:, 3:6], lam_h))
    with torch.cuda.stream(side):      # out= reuse: every entry is rewritten
        again = cam.trace_back_transmittance(rays, lam, out=T, screen=scr, flags=fl)
    side.synchronize()
    for a, b in zip(again, spectral):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the splat side on the same stream, with out= reuse
    m, k = 9, 257
    pts_h, u_h = pc.batch(pc.params_of("C3"), k), _u(k, m)
    with torch.cuda.stream(side):
        pts, u = torch.from_numpy(pts_h).to("cuda:0"), torch.from_numpy(u_h).to("cuda:0")
        bounds = cam.pupil_bounds(pts, G)
        out = torch.full((k, m), 7.0, dtype=torch.float32, device="cuda:0")
        res = cam.splat_transmittance(pts, bounds, u, out=out)
        fresh = cam.splat_transmittance(pts, bounds, u)
    side.synchronize()
    assert res.data_ptr() == out.data_ptr() and torch.equal(out.view(torch.int32), fresh.view(torch.int32)) and (out != 7.0).all().item()
    assert cam.counters() == after_forward
    assert first.tobytes() == cam.create_rays(smp, rng_states=st)["rays"].tobytes()
    # numpy in, numpy out
    Tn, sn, fn = cam.trace_back_transmittance(rays_h[:777], lam_h[:777])
    assert all(isinstance(a, np.ndarray) for a in (Tn, sn, fn))
    for a, t in zip((Tn, sn, fn), spectral):
        assert np.array_equal(a.view(np.uint32), t.cpu().numpy()[:777].view(np.uint32))
    assert np.array_equal(_bits(cam.splat_transmittance(pts_h, pupil_bounds_records(bounds), u_h)), _bits(out.cpu().numpy()))
    cam.close()


@pytest.mark.gpu
def test_argument_errors_leave_every_output_alone(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C3")
    n, m = 16, 4
    rays_h, lam_h = _batch(cam, p)
    rays = torch.from_numpy(rays_h[:n + 1].copy()).to("cuda:0")
    lam = torch.full((n + 1,), 550.0, dtype=torch.float32, device="cuda:0")
    T = torch.full((n + 1,), 7.0, dtype=torch.float32, device="cuda:0")
    scr = torch.full((n + 1, 2), 7.0, dtype=torch.float32, device="cuda:0")
    fl = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda:0")
    host = np.zeros((n, 8), F32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    R, L, Tp, S, Fp = rays.data_ptr(), lam.data_ptr(), T.data_ptr(), scr.data_ptr(), fl.data_ptr()
    d, s = lib.zoic_trace_back_transmittance_device, lib.zoic_trace_back_transmittance_spectral_device
    before = cam.counters()
    assert d(cam._h, n, None, Tp, S, Fp, st) == 1
    assert d(cam._h, n, R, None, S, Fp, st) == 1
    assert d(cam._h, n, R + 8, Tp, S, Fp, st) == 1                  # misaligned records
    assert d(cam._h, n, R, Tp + 2, S, Fp, st) == 1                  # misaligned d_transmittance
    assert d(cam._h, n, R, Tp, S + 4, Fp, st) == 1                  # misaligned d_screen
    assert d(cam._h, n, R, Tp, S, Fp + 2, st) == 1                  # misaligned d_flags
    assert d(cam._h, n, host.ctypes.data, Tp, S, Fp, st) == 1       # a host pointer
    assert d(cam._h, n, R, host.ctypes.data, S, Fp, st) == 1
    assert d(None, n, R, Tp, S, Fp, st) == 1
    assert d(cam._h, 0, None, None, None, None, st) == 0            # n = 0: no-op
    assert s(cam._h, n, R, None, Tp, S, Fp, st) == 1                # NULL d_wavelengths
    assert s(cam._h, n, R, L + 2, Tp, S, Fp, st) == 1
    assert s(cam._h, n, R, L, None, S, Fp, st) == 1
    assert s(cam._h, 0, None, None, None, None, None, st) == 0
    fresh = ZoicCamera(device=0)
    assert d(fresh._h, n, R, Tp, S, Fp, st) == 9 and s(fresh._h, n, R, L, Tp, S, Fp, st) == 9      # NOT_UPDATED
    fresh.close()
    # the splat side
    pts = torch.from_numpy(pc.batch(pc.params_of("C3"), n + 1)).to("cuda:0")
    u = torch.from_numpy(_u(n + 1, m)).to("cuda:0")
    bounds = cam.pupil_bounds(pts, G)
    out = torch.full((n + 1, m), 7.0, dtype=torch.float32, device="cuda:0")
    P, B, Uu, O = pts.data_ptr(), bounds.data_ptr(), u.data_ptr(), out.data_ptr()
    ds, ss = lib.zoic_splat_transmittance_device, lib.zoic_splat_transmittance_spectral_device
    assert ds(cam._h, n, P, B, 0, Uu, O, st) == 1 and ss(cam._h, n, P, B, L, 0, Uu, O, st) == 1      # m = 0 with n > 0
    assert ds(cam._h, n, None, B, m, Uu, O, st) == 1 and ds(cam._h, n, P, None, m, Uu, O, st) == 1
    assert ds(cam._h, n, P, B, m, None, O, st) == 1 and ds(cam._h, n, P, B, m, Uu, None, st) == 1
    assert ds(cam._h, n, P, B, m, Uu, O + 2, st) == 1 and ds(cam._h, n, P, B + 8, m, Uu, O, st) == 1
    assert ds(cam._h, n, P, B, m, Uu + 4, O, st) == 1 and ds(cam._h, n, P + 2, B, m, Uu, O, st) == 1
    assert ds(cam._h, n, P, B, m, Uu, host.ctypes.data, st) == 1
    assert ds(cam._h, 1 << 40, P, B, 1 << 20, Uu, O, st) == 1       # n m too large
    assert ss(cam._h, n, P, B, None, m, Uu, O, st) == 1 and ss(cam._h, n, P, B, L + 2, m, Uu, O, st) == 1
    assert ds(cam._h, 0, None, None, m, None, None, st) == 0 and ss(cam._h, 0, None, None, None, 0, None, None, st) == 0
    torch.cuda.synchronize()
    assert (T == 7.0).all().item() and (scr == 7.0).all().item() and (fl == -1).all().item() and (out == 7.0).all().item()
    assert cam.counters() == before
    # and nothing is written past n (n m)
    assert d(cam._h, n, R, Tp, S, Fp, st) == 0 and ds(cam._h, n, P, B, m, Uu, O, st) == 0
    torch.cuda.synchronize()
    assert T[n].item() == 7.0 and (scr[n] == 7.0).all().item() and fl[n].item() == -1 and (out[n] == 7.0).all().item()
    assert (T[:n] != 7.0).all().item() and (out[:n] != 7.0).all().item()
    cam.close()
    host_cam = tc.update(ZoicCamera(device=-1), tc.params_of("C3"))
    assert d(host_cam._h, n, R, Tp, S, Fp, st) == 11 and ds(host_cam._h, n, P, B, m, Uu, O, st) == 11      # NO_DEVICE
    host_cam.close()


@pytest.mark.gpu
def test_the_call_follows_updates_and_setters(gpu):
    cam, p = _camera("C3")
    cam.set_abbe_numbers(None)
    rays, lam = _batch(cam, p)
    rays, lam = rays[::4].copy(), np.ascontiguousarray(lam[::4])
    o, d = rays[:, 0:3], rays[:, 3:6]

    def check(w=None):
        got = cam.trace_back_transmittance(rays, wavelengths=w)
        assert _same(got, tr.lib_throughput(cam, o, d, w))
        return got[0]

    first = check()
    tr.coat(cam, _films(cam))                                              # new coatings: read at the call
    film = check()
    assert (film[first > 0] > first[first > 0]).mean() > 0.9
    tr.coat(cam, None)
    assert np.array_equal(_bits(check()), _bits(first))
    plain = check(lam)
    cam.set_abbe_numbers(np.full(cam.info()["lensCount"], 25.0, F32))      # new V-numbers: read at the call
    flint = check(lam)
    assert not np.array_equal(_bits(flint), _bits(plain)) and np.array_equal(_bits(check()), _bits(first))
    cam.set_abbe_numbers(None)
    tc.update(cam, dict(p, fStop=8.0))                                     # an update: the stop closes
    stopped = check()
    assert (stopped > 0).sum() < (first > 0).sum()
    p2 = tc.params_of("triplet")                                           # a new lens
    tc.update(cam, p2)
    assert not np.array_equal(_bits(check()), _bits(first))
    check(lam)
    tc.update(cam, tc.params_of("C1-vignetting"))                          # a thin lens: 1.0 where traced
    thin = check(lam)
    assert set(np.unique(thin).tolist()) <= {0.0, 1.0}
    cam.close()

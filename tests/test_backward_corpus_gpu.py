"""The four backward kernels on the MI355X over the pinned corpus of machine-made lenses (machine_lens_corpus.py: 5 ... 14 interfaces,
the stop at trace index 0, near-hemispherical rear elements, a camera outside the geometric domain):

  * zoic_trace_back_rays_device, zoic_trace_back_rays_spectral_device, zoic_project_points_device and
    zoic_project_points_spectral_device give their per-item host calls' bits, flags included, on every lens of the corpus -- no
    tolerance: the whole set, prefixes of 1, 63, 64 and 65 items and, for the lenses of the most and the fewest interfaces, one grid
    and one item (524 289, the set tiled); valid and rejected wavelengths interleaved inside one wave; at 587.5618 nm the spectral
    kernels give the d-line kernels' bits;
  * on the six accuracy lenses the records a FAST camera writes come back, on the buffer they were written to, within 5 x max E_ref
    (the yardstick of test_traceback_gpu.py::test_round_trip_on_the_device), and the records the STRICT spectral kernel writes at
    wavelengths uniform in [400, 700] nm within 2 x the same lens's d-line round trip
    (test_backward_spectral_gpu.py::test_round_trip_with_the_forward_spectral_kernel).

Each host side is a Python loop over the per-item C calls, so a lens is given at most 8192 rays (a stride of its live forward records,
the rejection families made from a stride of them, 1024 random lines, the non-finite rays: 5666 ... 6066 of them) and at most 2048
points (a stride of its kolb_point_set and six hostile points).  Measured on the host calls for these sets: 99.9 ... 100 % of the live
records are traced back, the refused rays end for all of the reasons 1 ... 5, and on the lens outside the domain every ray is refused
kTbOutsideDomain (7) and every point kRevOutsideDomain (5), a rejected wavelength (8 / 6) coming first.

The two round trips print their ratios (FAST round trip / max E_ref, spectral round trip / d-line round trip, the edge shares and the
control's median); the CPU-side yardsticks max E_ref are those of test_backward_corpus_cpu.py's table.  The device ratios have not been
recorded here: the bounds are the project's existing ones and do not depend on them.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT
from zoic_amd.workloads import ray_rng_states

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import traceback_cases as tc
from device_cases import bits as _bits
from machine_lens_corpus import EDGE_CAP, GRID_PLUS_ONE, PREFIXES
from traceback_cases import lib_project, lib_trace
from traceback_ref import OUTSIDE_DOMAIN

F32 = np.float32
REV_OUTSIDE = 5                   # kRevOutsideDomain (csrc/reverse.hpp)


def _ray_set(oracle_lib, cam, name):
    """a writable copy of the shared ray set (torch.from_numpy wants one) and the number of its leading live forward records"""
    rays, n_live = mc.ray_set(oracle_lib, cam, name)
    return np.array(rays), n_live


def _point_set(name):
    """a stride of the lens's kolb_point_set (petzval-2's for the lens outside the domain, which has none) and the hostile points"""
    pts = mc.point_set("petzval-2" if name == mc.OUTSIDE else name)[0]
    nan, inf = F32(np.nan), F32(np.inf)
    hostile = np.array([[0.1, 0.2, 1.0], [nan, 0, -10], [0, inf, -10], [0, 0, -5], [-0.0, -0.0, -5], [3, 1, -1e30]], F32)
    pts = np.ascontiguousarray(np.concatenate([mc.strided(pts, mc.MAX_POINTS - len(hostile)), hostile]), F32)
    assert len(pts) <= mc.MAX_POINTS
    return pts


def _batches(name, items, lam, call, host):
    """device == host on the whole set, on the prefixes and (two lenses) on one grid and one item, the set tiled"""
    import torch
    hs, hf = host
    scr, fl = call(items, lam)
    assert np.array_equal(_bits(scr), _bits(hs)) and np.array_equal(fl.astype(np.uint32), hf)
    for n in PREFIXES + ((GRID_PLUS_ONE,) if name in mc.LARGE_BATCH else ()):
        reps = -(-n // len(items))
        it = torch.from_numpy(np.tile(items, (reps, 1))[:n].copy()).to("cuda:0")
        lm = None if lam is None else torch.from_numpy(np.tile(lam, reps)[:n].copy()).to("cuda:0")
        s, f = call(it, lm)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s.cpu().numpy()), np.tile(_bits(hs), (reps, 1))[:n]), n
        assert np.array_equal(f.cpu().numpy().astype(np.uint32), np.tile(hf, reps)[:n]), n


def _trace_back(cam):
    return lambda r, w: cam.trace_back(r) if w is None else cam.trace_back(r, wavelengths=w)


def _project(cam):
    return lambda q, w: cam.project_points(q) if w is None else cam.project_points(q, wavelengths=w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_trace_back_kernel_equals_host_bitwise(gpu, oracle_lib, name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    rays, n_live = _ray_set(oracle_lib, cam, name)
    hs, hf = lib_trace(cam, rays[:, 0:3], rays[:, 3:6])
    refused = tc.reason(hf[(hf & 1) == 0])
    print("%s: %d rays, %d of %d live records traced back, reasons %s" % (name, len(rays), int((hf[:n_live] & 1).sum()), n_live, sorted(set(refused.tolist()))))
    if name == mc.OUTSIDE:
        assert cam.info()["fastRunsStrict"]
        assert (hf == OUTSIDE_DOMAIN << 8).all() and not _bits(hs).any()
    else:
        assert (hf[:n_live] & 1).sum() > 0.9 * n_live
        assert len(set(refused.tolist())) >= 3
    _batches(name, rays, None, _trace_back(cam), (hs, hf))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_spectral_trace_back_kernel_equals_host_bitwise(gpu, oracle_lib, name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    assert cam.dispersion()["cauchy_b"].any()
    rays, n_live = _ray_set(oracle_lib, cam, name)
    lam = bs.mixed_wavelengths(len(rays))
    hs, hf = lib_trace(cam, rays[:, 0:3], rays[:, 3:6], lam)
    good = bs.valid(lam)
    assert (hf[~good] == bs.TB_WAVELENGTH << 8).all() and not _bits(hs[~good]).any()
    if name == mc.OUTSIDE:
        assert (hf[good] == OUTSIDE_DOMAIN << 8).all() and not _bits(hs).any()
    else:
        assert (hf[:n_live][good[:n_live]] & 1).sum() > 1000
        assert len(set(tc.reason(hf[good & ((hf & 1) == 0)]).tolist())) >= 3
    _batches(name, rays, lam, _trace_back(cam), (hs, hf))
    # at the d-line: the d-line kernel's bits
    s0, f0 = cam.trace_back(rays)
    s1, f1 = cam.trace_back(rays, wavelengths=np.full(len(rays), bs.LAMBDA_D, F32))
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1)
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_projection_kernels_equal_host_bitwise(gpu, name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    pts = _point_set(name)
    lam = bs.mixed_wavelengths(len(pts))
    good = bs.valid(lam)
    host = lib_project(cam, pts)
    host_lam = lib_project(cam, pts, lam)
    print("%s: %d points, %d projected at the d-line, %d of %d at valid wavelengths" % (
        name, len(pts), int((host[1] & 1).sum()), int((host_lam[1][good] & 1).sum()), int(good.sum())))
    assert (host_lam[1][~good] == bs.PROJECT_WAVELENGTH << 8).all() and not _bits(host_lam[0][~good]).any()
    if name == mc.OUTSIDE:
        assert (host[1] == REV_OUTSIDE << 8).all() and not _bits(host[0]).any()
        assert (host_lam[1][good] == REV_OUTSIDE << 8).all() and not _bits(host_lam[0]).any()
    else:
        assert (host[1] & 1).sum() >= 0.9 * (len(pts) - 6) and (host_lam[1][good] & 1).sum() >= 0.9 * (good.sum() - 6)
        assert ((host[1] & 1) == 0).sum() >= 3    # (of the hostile points)
    _batches(name, pts, None, _project(cam), host)
    _batches(name, pts, lam, _project(cam), host_lam)
    s0, f0 = cam.project_points(pts)
    s1, f1 = cam.project_points(pts, wavelengths=np.full(len(pts), bs.LAMBDA_D, F32))
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1)
    cam.close()


def _yardstick(oracle_lib, name):
    """(host camera, params, samples, SpectralTraceBack, max E_ref): E_ref as test_traceback_gpu.py::test_round_trip_on_the_device takes
    it, from the oracle's records of the frame through the f64 trace-back"""
    s, o, d, w = mc.oracle_records(oracle_lib, name)
    host, p = mc.camera(name)
    T = bs.SpectralTraceBack(host.info(), p, host.dispersion())
    live = w > 0
    ref = T.trace(o[live], d[live])
    good = ref["traced"] & ~T.edge(ref)
    e_max = float(np.abs(ref["ps"] - s[live, :2].astype(np.float64)).max(1)[good].max())
    return host, p, s, T, e_max


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_round_trip_on_the_device(gpu, oracle_lib, name):
    """FAST camera: create_rays, then trace_back on the same device buffer and stream.  The edge set is the f64 trace-back's on the
    host copy of the FAST records."""
    import torch
    host, p, s, T, e_max = _yardstick(oracle_lib, name)
    cam, _ = mc.camera(name, device=0, precision=PRECISION_FAST)
    smp = torch.from_numpy(np.array(s)).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(tc.N).view(np.int32)).to("cuda:0")
    before = cam.counters()
    fwd = cam.create_rays(smp, rng_states=st)
    after = cam.counters()
    scr, fl = cam.trace_back(fwd)            # the dict create_rays returned: its buffer is read in place
    torch.cuda.synchronize()
    assert cam.counters() == after and after != before   # the forward call counts, the trace-back does not
    rec = fwd["rays"].cpu().numpy()
    scr, fl = scr.cpu().numpy(), fl.cpu().numpy().astype(np.uint32)
    live = rec[:, 6] > 0
    ref = T.trace(rec[live, 0:3], rec[live, 3:6])
    edge = T.edge(ref)
    assert live.sum() >= 4096 and edge.mean() <= EDGE_CAP, (live.sum(), edge.mean())
    ok = (fl[live] & 1) == 1
    assert ok[~edge].all(), ((~ok & ~edge).sum(), np.unique(tc.reason(fl[live][~ok & ~edge])))
    rt = np.abs(scr[live].astype(np.float64) - s[live, :2].astype(np.float64)).max(1)[~edge]
    print("%s FAST round trip: live %d, max %.3g = %.2f x max E_ref (%.3g); edge share %.2f %%" % (
        name, live.sum(), rt.max(), rt.max() / e_max, e_max, 100 * edge.mean()))
    assert rt.max() <= 5.0 * e_max, (rt.max(), e_max, rt.max() / e_max)
    cam.close()
    host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_spectral_round_trip_on_the_device(gpu, oracle_lib, name):
    """STRICT camera, wavelengths uniform in [400, 700] nm per ray: create_rays(samples, wavelengths) then trace_back(rays, wavelengths)
    on the same stream and buffer.  Every record of weight > 0 outside the edge set comes back, within 2 x the d-line round trip's
    maximum, measured here with the d-line calls on the same samples.  The edge set is TraceBack.edge's on the f64 restatement of the
    records at their wavelengths rounded to whole nanometres.  Control: the d-line trace-back of the same spectral records misses, in
    the median, by more than the spectral round trip's maximum (every corpus lens has colour)."""
    import torch
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    host, _ = mc.camera(name)
    disp = host.dispersion()
    T = bs.SpectralTraceBack(host.info(), p, disp)
    n = tc.N
    s = np.array(mc.oracle_records(oracle_lib, name)[0])
    smp = torch.from_numpy(s).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(n).view(np.int32)).to("cuda:0")
    lam_h = np.random.default_rng(23).uniform(400.0, 700.0, n).astype(F32)
    lam = torch.from_numpy(lam_h).to("cuda:0")
    # the d-line round trip of the d-line calls on the same samples: the yardstick
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
    assert live.sum() >= 4096 and edge.mean() <= EDGE_CAP, (live.sum(), edge.mean())
    ok = (fl[live] & 1) == 1
    assert ok[~edge].all(), ((~ok & ~edge).sum(), np.unique(tc.reason(fl[live][~ok & ~edge])))
    rt = np.abs(scr[live].astype(np.float64) - s[live, :2]).max(1)[~edge]
    c_ok = ~edge & ((cfl.cpu().numpy()[live] & 1) == 1)
    control = np.abs(ctl.cpu().numpy()[live].astype(np.float64) - s[live, :2]).max(1)[c_ok]
    print("%s spectral round trip: live %d, edge share %.2f %%, max %.3g = %.2f x the d-line round trip's max (%.3g); control (d-line "
          "trace-back of the spectral records): median %.3g" % (name, live.sum(), 100 * edge.mean(), rt.max(), rt.max() / d_max, d_max, np.median(control)))
    assert rt.max() <= 2.0 * d_max, (rt.max(), d_max)
    if disp["cauchy_b"].any():
        assert np.median(control) > rt.max(), (np.median(control), rt.max())
    cam.close()
    host.close()

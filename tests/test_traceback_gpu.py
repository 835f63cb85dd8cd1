"""Trace-back on the MI355X (zoic_trace_back_rays_device): the batch kernel gives zoic_trace_back_ray's bits, flags included,
deterministically and whatever the batch size; the records a FAST camera writes are taken back, on the device buffer they were
written to, to the samples they were made from; the call writes into the caller's tensors, refuses bad pointers before any launch,
leaves the counters alone and is ordered on its stream."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states, synthetic_samples

import traceback_cases as tc
from device_cases import records as _records
from traceback_ref import TraceBack

SLAB = 2048 * 256   # one grid of the kernel (kPassGridCap x kPassBlock, device_pass.hpp): larger batches are walked slab by slab
W, H, SPP = 256, 144, 2   # 73 728 rays


def _camera(cfg, precision=PRECISION_STRICT, **over):
    p = dict(camera_params(cfg), **over)
    cam = ZoicCamera(device=0)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    cam.set_precision(precision)
    cam.update(**p)
    return cam, p


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_kernel_equals_host_bitwise(gpu, cfg):
    import torch
    cam, p = _camera(cfg)
    n = W * H * SPP
    fwd = cam.create_rays(synthetic_samples(n, W, H, SPP), rng_states=ray_rng_states(n))
    rec = np.ascontiguousarray(fwd["rays"]).view(np.float32).reshape(-1, 8)   # every record, whatever its weight
    info = cam.info()
    live = np.flatnonzero(fwd["weight"] > 0)[::16]
    sets = [rec, _records(*tc.non_finite_rays()), _records(*tc.random_lines(info, 4096))]
    edge = np.array([[0, 0, -1, 0, 0, -1], [0, 0, -1e30, 0, 0, -1e-30], [1e30, 0, -1, 0, 0, -1], [0, 0, -1, 1e30, 0, -1e-30],
                     [0, 0, 0, 0, 0, -1], [-0.0, -0.0, -0.0, -0.0, -0.0, -1], [0, 0, -1, 1, 0, -1e-38], [1e-30, 1e-30, -1e-30, 1e-30, 0, -1e-30]],
                    np.float32)
    sets.append(_records(edge[:, :3], edge[:, 3:]))
    if p["lensModel"] == _capi.RAYTRACED:
        fam = tc.rejection_families(info, rec[live, 0:3], rec[live, 3:6])
        sets += [_records(o, d) for o, d in fam.values()]
    rays = np.ascontiguousarray(np.concatenate(sets), dtype=np.float32)
    scr, fl = cam.trace_back(rays)
    hs, hf = tc.lib_trace(cam, rays[:, 0:3], rays[:, 3:6])
    assert np.array_equal(scr.view(np.uint32), hs.view(np.uint32))
    assert np.array_equal(fl.astype(np.uint32), hf)
    assert (hf & 1).sum() > (fwd["weight"] > 0).sum() * 0.9
    assert len(set(tc.reason(hf[hf & 1 == 0]).tolist())) >= (3 if p["lensModel"] == _capi.RAYTRACED else 2)
    # twice: the same bits; then n = 1, 777 and more than one slab (tiled), each a prefix / tiling of the same rays
    scr2, fl2 = cam.trace_back(rays)
    assert np.array_equal(scr2.view(np.uint32), scr.view(np.uint32)) and np.array_equal(fl2, fl)
    for k in (1, 777):
        s, f = cam.trace_back(rays[:k])
        assert np.array_equal(s.view(np.uint32), scr[:k].view(np.uint32)) and np.array_equal(f, fl[:k])
    reps = SLAB // len(rays) + 2
    big = torch.from_numpy(np.tile(rays, (reps, 1))).to("cuda:0")
    s, f = cam.trace_back(big)
    torch.cuda.synchronize()
    assert big.shape[0] > SLAB
    assert np.array_equal(s.cpu().numpy().view(np.uint32), np.tile(scr, (reps, 1)).view(np.uint32))
    assert np.array_equal(f.cpu().numpy(), np.tile(fl, reps))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C2", "C3", "C4", "C5"])
def test_round_trip_on_the_device(gpu, oracle_lib, name):
    """FAST camera: create_rays, then trace_back on the same device buffer.  The yardstick E_ref is measured as the CPU test measures
    it (the oracle's records of the same frame through the f64 trace-back); the edge set is the f64 trace-back's on the host copy of
    the FAST records."""
    import torch
    p = tc.params_of(name)
    s, o, d, w = tc.oracle_records(oracle_lib, p)
    host = tc.update(ZoicCamera(device=-1), p)
    T = TraceBack(host.info(), p)
    live = w > 0
    ref = T.trace(o[live], d[live])
    good = ref["traced"] & ~T.edge(ref)
    e_max = float(np.abs(ref["ps"] - s[live, :2].astype(np.float64)).max(1)[good].max())
    host.close()

    cam, _ = _camera(tc.CONFIGS[name][0], PRECISION_FAST, **tc.CONFIGS[name][1])
    smp = torch.from_numpy(s).to("cuda:0")
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
    assert edge.mean() <= 0.02, edge.mean()
    ok = (fl[live] & 1) == 1
    assert ok[~edge].all(), ((~ok & ~edge).sum(), np.unique(tc.reason(fl[live][~ok & ~edge])))
    rt = np.abs(scr[live].astype(np.float64) - s[live, :2].astype(np.float64)).max(1)[~edge]
    print("%s FAST round trip: max %.3g = %.2f x max E_ref (%.3g); edge share %.2f %%" % (name, rt.max(), rt.max() / e_max, e_max, 100 * edge.mean()))
    assert rt.max() <= 5.0 * e_max, (rt.max(), e_max, rt.max() / e_max)
    cam.close()


@pytest.mark.gpu
def test_outputs_pointers_and_counters(gpu):
    import torch
    lib = _capi.load()
    cam, p = _camera("C2")
    n = 4096
    smp = torch.from_numpy(synthetic_samples(n, 64, 64, 1)).to("cuda:0")
    fwd = cam.create_rays(smp)
    rays = fwd["rays"]
    scr, fl = cam.trace_back(rays)
    out = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda:0")
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    before = cam.counters()
    o2, f2 = cam.trace_back(rays, out=out, flags=flags)
    torch.cuda.synchronize()
    assert o2.data_ptr() == out.data_ptr() and f2.data_ptr() == flags.data_ptr()
    assert torch.equal(out, scr) and torch.equal(flags, fl) and (fl & 1).sum().item() > n // 2
    assert cam.counters() == before
    st = torch.cuda.current_stream().cuda_stream
    call = lib.zoic_trace_back_rays_device
    out.fill_(7.0)
    assert call(cam._h, n, rays.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 0      # flags may be NULL
    torch.cuda.synchronize()
    assert torch.equal(out, scr)
    host = np.zeros((n, 8), np.float32)
    assert call(cam._h, n, None, out.data_ptr(), None, C.c_void_p(st)) == 1
    assert call(cam._h, n, rays.data_ptr(), None, None, C.c_void_p(st)) == 1
    assert call(cam._h, n, host.ctypes.data, out.data_ptr(), None, C.c_void_p(st)) == 1      # not device memory
    assert call(cam._h, n - 1, rays.data_ptr() + 8, out.data_ptr(), None, C.c_void_p(st)) == 1   # misaligned records
    assert call(cam._h, n - 1, rays.data_ptr(), out.data_ptr() + 4, None, C.c_void_p(st)) == 1   # misaligned screen
    assert call(cam._h, n - 1, rays.data_ptr(), out.data_ptr(), flags.data_ptr() + 2, C.c_void_p(st)) == 1
    assert call(cam._h, 0, None, None, None, C.c_void_p(st)) == 0                            # n = 0: no-op
    fresh = ZoicCamera(device=0)
    assert call(fresh._h, n, rays.data_ptr(), out.data_ptr(), None, C.c_void_p(st)) == 9     # NOT_UPDATED
    fresh.close()
    # numpy records in, numpy out
    rec = np.ascontiguousarray(rays.cpu().numpy()).view(_capi.RAY_DTYPE).reshape(-1)
    s3, f3 = cam.trace_back(rec)
    assert np.array_equal(s3, scr.cpu().numpy()) and np.array_equal(f3, fl.cpu().numpy())
    cam.close()


@pytest.mark.gpu
def test_asynchronous_and_ordered_on_a_side_stream(gpu):
    import torch
    cam, p = _camera("C3")
    n = 1 << 20
    smp = torch.from_numpy(synthetic_samples(n, 1024, 512, 2)).to("cuda:0")
    want_rays = cam.create_rays(smp)["rays"].clone()
    want_scr, want_fl = cam.trace_back(want_rays)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    # queued behind a forward call on the same stream: the trace-back must see the records that call writes
    cam.create_rays(smp, out=dict(rays=rays), stream=side.cuda_stream)
    scr, fl = cam.trace_back(rays, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(rays, want_rays)
    assert torch.equal(scr, want_scr) and torch.equal(fl, want_fl)
    cam.close()

"""The trace-back Jacobian kernels on the MI355X over the pinned corpus of machine-made lenses (machine_lens_corpus.py) and far start
points, after test_backward_corpus_gpu.py:

  * zoic_trace_back_jacobian_device and zoic_trace_back_jacobian_spectral_device give the per-item host calls' bits -- Ps, flags and all
    twelve words of J, no tolerance -- on every lens of the corpus: the corpus ray set machine_lens_corpus.ray_set and 1 024 far rays
    (live records moved 30 ... 1e4 cm out along the ray, half of them with dir scaled by 1e3 or 1e-3; traceback_jacobian_ref.far_rays),
    at most 8 192 rays a lens; the whole set, prefixes of 1, 63, 64 and 65 items and, for the lenses of the most and the fewest
    interfaces, one grid and one item (524 289, the set tiled); valid and rejected wavelengths interleaved inside one wave; Ps and flags
    are those of the trace-back kernels; at 587.5618 nm the spectral kernel gives the d-line kernel's J; the lens outside the
    geometric domain refuses everything and writes zeros;
  * on the six accuracy lenses J composed with the forward differentials of a FAST camera is the identity within 1.5 x the residual of
    the f32 finite-difference Jacobian, as test_traceback_jacobian_gpu.py::test_round_trip_against_the_forward_differentials takes it,
    the yardstick's step being the one test_traceback_jacobian_corpus_cpu.py finds best for the lens.

Measured on the MI355X, the round trip (512 yardstick rays of the 64 x 36 x 2 frame; J's residual over the yardstick's, bound 1.5):

    lens        rays   |J T - I| median / p99   finite differences, h, median / p99   ratios
    triplet-4    507   1.42e-6 / 3.93e-6        2^-9   1.48e-4 / 4.87e-4              0.0096 / 0.0081
    fisheye-5    504   3.41e-6 / 1.07e-5        2^-13  9.60e-4 / 4.35e-3              0.0036 / 0.0025
    mori-6       497   2.73e-6 / 7.44e-6        2^-10  4.27e-4 / 1.71e-3              0.0064 / 0.0044
    double-3     506   6.72e-7 / 2.13e-6        2^-8   3.56e-5 / 1.25e-4              0.019  / 0.017
    tessar-5     497   9.86e-7 / 3.24e-6        2^-9   1.65e-4 / 6.05e-4              0.0060 / 0.0054
    petzval-2    508   3.51e-7 / 1.01e-6        2^-11  1.07e-4 / 3.13e-4              0.0033 / 0.0032

The bitwise comparisons find no differing word on any lens, d-line or spectral.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import traceback_cases as tc
import traceback_jacobian_ref as jr
from device_cases import bits as _bits, records as _records
from machine_lens_corpus import GRID_PLUS_ONE, PREFIXES, ray_set as _ray_set
from traceback_jacobian_ref import H, N, SPP, W, residual as _residual
from traceback_ref import OUTSIDE_DOMAIN

F32 = np.float32
FAR = 1024
# the yardstick's step per lens: the one tests/test_traceback_jacobian_corpus_cpu.py finds best for it (near, d-line)
YARDSTICK_H = {"triplet-4": 2.0 ** -9, "fisheye-5": 2.0 ** -13, "mori-6": 2.0 ** -10, "double-3": 2.0 ** -8, "tessar-5": 2.0 ** -9,
               "petzval-2": 2.0 ** -11}


def _rays(oracle_lib, cam, name):
    """(records (m,8) f32, how many of the last are the far ones): the corpus ray set, then the far rays made from the lens's live
    forward records"""
    rays, _ = _ray_set(oracle_lib, cam, name)
    _, o, d, w = mc.oracle_records(oracle_lib, name)
    far = _records(*jr.far_rays(o[w > 0], d[w > 0], FAR))
    out = np.ascontiguousarray(np.concatenate([rays, far]), F32)
    assert len(out) <= mc.MAX_RAYS and len(far) == FAR
    return out, len(far)


def _batches(cam, name, rays, lam, host):
    """device == host on the whole set, on the prefixes and (two lenses) on one grid and one item, the set tiled"""
    import torch
    hs, hf, hj = host
    scr, fl, jac = cam.trace_back_jacobian(rays, wavelengths=lam)
    assert jac.shape == (len(rays), 2, 6) and jac.dtype == np.float32
    assert np.array_equal(_bits(scr), _bits(hs)) and np.array_equal(fl.astype(np.uint32), hf) and np.array_equal(_bits(jac), _bits(hj))
    s0, f0 = cam.trace_back(rays, wavelengths=lam)   # the trace-back kernels' Ps and flags
    assert np.array_equal(_bits(s0), _bits(scr)) and np.array_equal(f0, fl)
    for n in PREFIXES + ((GRID_PLUS_ONE,) if name in mc.LARGE_BATCH else ()):
        reps = -(-n // len(rays))
        it = torch.from_numpy(np.tile(rays, (reps, 1))[:n].copy()).to("cuda:0")
        lm = None if lam is None else torch.from_numpy(np.tile(lam, reps)[:n].copy()).to("cuda:0")
        s, f, j = cam.trace_back_jacobian(it, wavelengths=lm)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s.cpu().numpy()), np.tile(_bits(hs), (reps, 1))[:n]), n
        assert np.array_equal(f.cpu().numpy().astype(np.uint32), np.tile(hf, reps)[:n]), n
        assert np.array_equal(_bits(j.cpu().numpy()), np.tile(_bits(hj), (reps, 1, 1))[:n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_jacobian_kernel_equals_host_bitwise(gpu, oracle_lib, name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    rays, n_far = _rays(oracle_lib, cam, name)
    hs, hf, hj = jr.host_jacobian(cam, rays[:, 0:3], rays[:, 3:6])
    traced = (hf & 1) == 1
    print("%s: %d rays, %d traced back, %d of the %d far ones; reasons %s" % (
        name, len(rays), traced.sum(), traced[-n_far:].sum(), n_far, sorted(set(tc.reason(hf[~traced]).tolist()))))
    assert not _bits(hj[~traced]).any()
    if name == mc.OUTSIDE:
        assert (hf == OUTSIDE_DOMAIN << 8).all() and not _bits(hs).any() and not _bits(hj).any()
    else:
        assert traced[-n_far:].sum() > 0.5 * n_far and len(set(tc.reason(hf[~traced]).tolist())) >= 3
        assert np.isfinite(hj[-n_far:][traced[-n_far:]]).all()
    _batches(cam, name, rays, None, (hs, hf, hj))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_spectral_jacobian_kernel_equals_host_bitwise(gpu, oracle_lib, name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    assert cam.dispersion()["cauchy_b"].any()
    rays, n_far = _rays(oracle_lib, cam, name)
    lam = bs.mixed_wavelengths(len(rays))
    good = bs.valid(lam)
    hs, hf, hj = jr.host_jacobian(cam, rays[:, 0:3], rays[:, 3:6], lam)
    traced = (hf & 1) == 1
    assert (hf[~good] == bs.TB_WAVELENGTH << 8).all() and not _bits(hs[~good]).any() and not _bits(hj[~traced]).any()
    if name == mc.OUTSIDE:
        assert (hf[good] == OUTSIDE_DOMAIN << 8).all() and not _bits(hs).any() and not _bits(hj).any()
    else:
        assert traced[-n_far:].sum() > 0.3 * n_far and len(set(tc.reason(hf[good & ~traced]).tolist())) >= 3
    _batches(cam, name, rays, lam, (hs, hf, hj))
    # at the d-line: the d-line kernel's bits, J included
    s0, f0, j0 = cam.trace_back_jacobian(rays)
    s1, f1, j1 = cam.trace_back_jacobian(rays, wavelengths=np.full(len(rays), bs.LAMBDA_D, F32))
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1) and np.array_equal(_bits(j0), _bits(j1))
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_round_trip_against_the_forward_differentials(gpu, oracle_lib, name):
    """test_traceback_jacobian_gpu.py's round trip on a corpus lens: FAST camera, T = [dOdx dOdy; dDdx dDdy] of the forward
    differentials, |J T - I|_max of the kernel's J within 1.5 x that of the f32 finite-difference Jacobian (median and p99, 512 rays,
    the finite differences taken one front housing radius out on the same line and brought back)."""
    import torch
    from traceback_ref import TraceBack
    cam, p = mc.camera(name, device=0, precision=PRECISION_FAST)
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
    print("%s: %d rays; |J T - I| median %.3g p99 %.3g; finite differences median %.3g p99 %.3g; ratios %.3g / %.3g" % (
        name, len(pick), np.median(rj), np.percentile(rj, 99), np.median(ry), np.percentile(ry, 99), np.median(rj) / np.median(ry),
        np.percentile(rj, 99) / np.percentile(ry, 99)))
    assert np.median(rj) <= 1.5 * np.median(ry), (np.median(rj), np.median(ry))
    assert np.percentile(rj, 99) <= 1.5 * np.percentile(ry, 99), (np.percentile(rj, 99), np.percentile(ry, 99))
    cam.close()

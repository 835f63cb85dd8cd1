"""Traced ray differentials of spectral records on the MI355X (zoic_ray_differentials_spectral_device) over the pinned corpus of
machine-made lenses (machine_lens_corpus.py), after tests/test_differentials_spectral_corpus_cpu.py, with which these tests share the
frame, wavelengths, reference, conditioning rule and groups of differentials_spectral_corpus.py:

  A  on the accuracy group a STRICT camera's screen tangents and wavelength tangent against the f64 reference started from the
     records' own tries -- the tries the spectral forward kernel accepted at each ray's wavelength -- within
     test_differentials_spectral_gpu's bounds, the reference-only conditions asserted first;
  B  the kernel against the host build of csrc/differentials_spectral.hpp from the same starts on every lens but petzval-5: within
     test_host_equals_device's bounds on the accuracy group, within 2 x the d-line kernel's own distance from its host build (same
     lens, same start rays) on the identities-only lenses;
  C  the identities the header promises, bit for bit, on all ten lenses;
  D  on the accuracy group the spectral trace-back Jacobian composed with the spectral forward differentials is the identity within
     2 x the d-line round trip's residual of the same lens, rays and run.

Measured on the MI355X (the frame traceback_cases.frame_samples(), 41 472 rays; median / 99.9th percentile unless named).

A, STRICT against f64; no ray is left out by the conditioning rule (excluded share 0 on every lens); restatement eo / ed medians
3.6e-7 ... 8.0e-7 / 1.2e-7 ... 1.8e-7:

    lens       rays  retried  screen tangents       against its contributions   against its own size    cancellation
    triplet-4  3753   238     1.72e-07 / 4.20e-06   5.04e-09 / 5.24e-08         2.54e-08 / 7.92e-08      7.9
    fisheye-5  3903  1137     2.25e-07 / 1.07e-06   8.29e-09 / 4.33e-08         2.56e-08 / 8.25e-08      3.3
    mori-6     4001   320     5.58e-07 / 4.85e-06   3.12e-09 / 1.40e-08         2.53e-08 / 7.76e-08      7.0
    double-3   3858  1170     2.79e-07 / 1.42e-06   7.51e-09 / 4.48e-08         2.54e-08 / 7.62e-08      3.4
    tessar-5   3802  1001     2.25e-07 / 2.93e-06   9.04e-10 / 4.37e-09         2.55e-08 / 8.54e-08     20.8
    petzval-2  3656  1436     2.70e-07 / 1.95e-06   1.72e-09 / 7.43e-09         2.54e-08 / 7.72e-08     15.3

B, the kernel against the host build; the wavelength tangent is the host's bit for bit on every lens (IEEE f64 on both sides):

    lens       rays  retried  spectral, driver mode 2   d-line, driver mode 0   ratios (bound 2 on the last three)
    triplet-4  3736   237     1.43e-07 / 4.70e-06       1.34e-07 / 4.71e-06     1.06 / 1.00
    fisheye-5  3886  1100     2.84e-07 / 1.14e-06       2.81e-07 / 1.17e-06     1.01 / 0.97
    mori-6     3996   318     6.40e-07 / 6.10e-06       6.34e-07 / 6.66e-06     1.01 / 0.92
    double-3   3959  1220     3.14e-07 / 1.60e-06       3.13e-07 / 1.68e-06     1.01 / 0.95
    tessar-5   3814   979     2.21e-07 / 3.18e-06       2.20e-07 / 3.10e-06     1.00 / 1.03
    petzval-2  3630  1463     3.03e-07 / 2.20e-06       3.02e-07 / 2.24e-06     1.01 / 0.98
    mori-4     3904     9     6.98e-07 / 4.49e-05       7.04e-07 / 4.01e-05     0.99 / 1.12
    rear-9     3795  2876     2.84e-07 / 6.62e-06       2.90e-07 / 6.47e-06     0.98 / 1.02
    rear-12    3884  2586     3.07e-07 / 3.12e-06       3.03e-07 / 3.02e-06     1.01 / 1.03

C: no differing word on any lens; the STRICT and the FAST camera's records agree on every row of every lens (petzval-5 runs STRICT).

D, |J T - I|_max on 512 rays of the 64 x 36 x 2 frame, FAST (median / 99th percentile; bound on the ratios 2):

    lens       spectral               d-line, same rays and run   ratios
    triplet-4  1.17e-06 / 3.50e-06    1.40e-06 / 3.70e-06         0.84 / 0.95
    fisheye-5  3.52e-06 / 1.27e-05    3.39e-06 / 1.03e-05         1.04 / 1.23
    mori-6     2.79e-06 / 9.16e-06    2.60e-06 / 7.80e-06         1.07 / 1.17
    double-3   8.13e-07 / 2.25e-06    6.27e-07 / 2.03e-06         1.30 / 1.11
    tessar-5   1.15e-06 / 3.32e-06    9.52e-07 / 3.07e-06         1.21 / 1.08
    petzval-2  4.18e-07 / 1.23e-06    3.76e-07 / 9.89e-07         1.11 / 1.25
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import differentials_ref as dref
import differentials_spectral_ref as sref
import machine_lens_corpus as mc
import host_drivers
import traceback_jacobian_ref as jr
from device_cases import BIG, bits as _bits, spectral_run as _run
from differentials_spectral_corpus import (ACCURACY, HOST_DEVICE, IDENTITIES_ONLY, conditions, figures, frame, line, reference, reference_rows, tables,
                                           wave_with as _wave_with)
from fuzz_cameras import MachineLens, rows_of
from host_drivers import run_differentials_spectral as run_driver
from machine_lens_corpus import EDGE_CAP, PREFIXES
from spectral_ref import BAD, LAMBDA_D32

pytestmark = pytest.mark.gpu

F32 = np.float32
SPLIT = [0, 1, 64, 5037]


def _tries(rays):
    return ((rays[:, 7].view(np.uint32) >> 1) & 31).astype(np.int64)


def _frame():
    """writable copies of the shared frame (torch.from_numpy wants them)"""
    return tuple(np.array(a) for a in frame())


_LAUNCH = {}


def _launch(name):
    """One STRICT launch of the frame at its wavelengths behind lens `name`: (records (N,8), differentials (N,12), chroma (N,6)) and the
    d-line records and differentials of the same samples and streams"""
    if name not in _LAUNCH:
        import torch
        cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
        assert cam.dispersion()["cauchy_b"].any()
        s, st, lam = _frame()
        spectral = _run(cam, s, lam, states=st)
        ts, tst = torch.from_numpy(s).cuda(), torch.from_numpy(st.view(np.int32)).cuda()
        rays0 = cam.create_rays(ts, rng_states=tst)["rays"]
        diffs0 = cam.ray_differentials(ts, rays0, rng_states=tst)
        torch.cuda.synchronize()
        _LAUNCH[name] = spectral + (rays0.cpu().numpy(), diffs0.cpu().numpy())
        cam.close()
    return _LAUNCH[name]


def _starts(oracle_lib, name, rays, rows):
    """(surfaces, o0, d0) of the rows `rows` of the records `rays`: differentials_ref.kolb_start on the records' own tries"""
    p = tables(name)[0]
    s, st, _ = frame()
    oc = mc.oracle_camera(oracle_lib, name)
    surf = dref.surfaces(oc.lens_table())
    o0, d0 = dref.kolb_start(oc, p, s[rows], _tries(rays)[rows], st[rows], oracle_lib)
    oc.close()
    return surf, o0, d0


_REF = {}


def _device_reference(oracle_lib, name):
    """The f64 reference of the spectral launch's records, reference_rows of the live ones: start rays from the records' tries, the
    restatement of the records at their wavelengths, the conditions -- nothing of the differentials is read here"""
    if name not in _REF:
        rays = _launch(name)[0]
        p, info, disp, hs = tables(name)
        lam = frame()[2]
        rows = reference_rows(np.flatnonzero(rays[:, 6] != 0), _tries(rays))
        surf, o0, d0 = _starts(oracle_lib, name, rays, rows)
        ref = reference(surf, disp, hs, lam[rows], o0, d0)
        ro, rd = ref["end"]
        eo = np.linalg.norm(-ro - rays[rows, 0:3], axis=1) / np.linalg.norm(rays[rows, 0:3], axis=1)
        ed = np.linalg.norm(-rd - rays[rows, 3:6], axis=1) / np.linalg.norm(rays[rows, 3:6], axis=1)
        _REF[name] = dict(rows=rows, surf=surf, o0=o0, d0=d0, lam=np.array(lam[rows]), ref=ref, eo=eo, ed=ed,
                          retried=int((_tries(rays)[rows] > 0).sum()))
    return _REF[name]


# ---- A: against f64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCURACY)
def test_spectral_differentials_correct(gpu, oracle_lib, name):
    """STRICT; the reference from the records' own tries (the spectral forward kernel's, at each ray's wavelength).  First, on the
    reference alone: the f64 restatement reproduces the records, the conditioning rule leaves out at most EDGE_CAP of the live rays,
    200 retried live rays are in the set.  Then the library: finite on every live row, +0.0 on every dead one; screen tangents median
    <= 1e-5 and 99.9 % within 1e-3; wavelength tangent at most 4 x the screen figures, against the sum of its contributions and against
    its own size."""
    R = _device_reference(oracle_lib, name)
    good, excluded, restated = conditions(R["ref"]["cos"], R["eo"], R["ed"])
    print("%-10s rows %4d  excluded %.4f  restatement %s (eo %.2e, ed %.2e / %.2e)  retried %d" % (
        name, len(R["rows"]), excluded, restated, np.median(R["eo"]), np.median(R["ed"]), np.percentile(R["ed"], 99.9), R["retried"]))
    assert dref.restatement_holds(R["eo"], R["ed"]) and restated, (float(np.median(R["eo"])), float(np.median(R["ed"])))
    assert excluded <= EDGE_CAP, (name, excluded)
    assert R["retried"] >= 200, "only %d retried live rays" % R["retried"]
    rays, diffs, chroma = _launch(name)[:3]
    dead = rays[:, 6] == 0
    assert np.isfinite(diffs[~dead]).all() and np.isfinite(chroma[~dead]).all()
    assert not _bits(diffs[dead]).any() and not _bits(chroma[dead]).any()
    m = figures(diffs[R["rows"]], chroma[R["rows"]], R["ref"], good)
    print("device  " + line(name, m, excluded))
    assert m["s_med"] <= 1e-5 and m["s_ok"] >= 0.999, m
    assert m["c_med"] <= 4 * m["s_med"] and m["c_tail"] <= 4 * m["s_tail"], m
    assert m["l_med"] <= 4 * m["s_med"] and m["l_tail"] <= 4 * m["s_tail"], m


# ---- B: against the host build ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return host_drivers.differentials_spectral()


@pytest.mark.parametrize("name", HOST_DEVICE)
def test_kernel_against_the_host_build(gpu, oracle_lib, driver, name):
    """The host build of csrc/differentials_spectral.hpp from the start rays kolb_start rebuilds through the oracle, against the kernel
    (not bitwise: diff_rsqrt / diff_sqrt / diff_rcp are 1-ulp instructions on the device).  The rows are those live in the spectral AND
    in the d-line launch with the same try count, so that both kernels differentiate the SAME start rays.

    The wavelength tangent, every lens: within test_host_equals_device's bounds against the sum of its contributions (median <= 1e-5,
    99.9 % within 1e-3).  It is an f64 trace of the same f32 start and tables on both sides, so this holds whatever the conditioning.
    Screen tangents, accuracy group: test_host_equals_device's bounds (median <= 1e-5, 99.9 % within 1e-3), the primal allclose to the
    records.  Screen tangents, identities-only lenses: the yardstick is the d-line kernel against driver mode 0 on the same rays; the
    spectral kernel against driver mode 2 may miss by 2 x that, median and 99.9th percentile (the margin the backward corpus gives a
    spectral round trip over its d-line one)."""
    rays, diffs, chroma, rays0, diffs0 = _launch(name)
    p, info, disp, hs = tables(name)
    lam = frame()[2]
    both = (rays[:, 6] != 0) & (rays0[:, 6] != 0) & (_tries(rays) == _tries(rays0))
    rows = reference_rows(np.flatnonzero(both), _tries(rays))
    assert len(rows) >= 2048
    surf, o0, d0 = _starts(oracle_lib, name, rays, rows)
    out, ch, prim = run_driver(driver, 2, surf, disp, hs, lam[rows], o0, d0)
    out0, _, _ = run_driver(driver, 0, surf, disp, hs, lam[rows], o0, d0)
    e = dref.rel_err(diffs[rows], out)
    e0 = dref.rel_err(diffs0[rows], out0)
    part = sref.wavelength_contributions(surf, disp, lam[rows], o0, d0)
    ec = np.linalg.norm((chroma[rows].astype(np.float64) - ch).reshape(-1, 2, 3), axis=2) / part
    f = dict(med=float(np.median(e)), tail=float(np.percentile(e, 99.9)), med0=float(np.median(e0)), tail0=float(np.percentile(e0, 99.9)))
    print("%-10s host vs device, %4d rays (%d retried): spectral %.2e / %.2e, d-line %.2e / %.2e, ratios %.2f / %.2f; wavelength tangent "
          "%.2e / max %.2e" % (name, len(rows), (_tries(rays)[rows] > 0).sum(), f["med"], f["tail"], f["med0"], f["tail0"],
                               f["med"] / max(f["med0"], 1e-300), f["tail"] / max(f["tail0"], 1e-300), np.median(ec), ec.max()))
    assert np.isfinite(diffs[rows]).all() and np.isfinite(chroma[rows]).all()
    assert np.median(ec) <= 1e-5 and (ec <= 1e-3).mean() >= 0.999
    if name in ACCURACY:
        assert np.allclose(prim, rays[rows, 0:6], rtol=1e-5, atol=1e-5)
        assert f["med"] <= 1e-5 and (e <= 1e-3).mean() >= 0.999, f
    else:
        assert name in IDENTITIES_ONLY
        assert f["med"] <= 2 * f["med0"] and f["tail"] <= 2 * f["tail0"], f


# ---- C: exact identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_d_line_and_flag_identities(gpu, name):
    """all wavelengths 587.5618: the 12 floats are ray_differentials' without wavelengths and the wavelength tangent is not all zero
    (every corpus lens has colour); chromatic on / off: the same 12 floats; two runs are equal; dsx / dsy scale the screen fields only.
    Valid and rejected wavelengths alternate inside every wave (bs.mixed_wavelengths)."""
    import torch
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    assert cam.dispersion()["cauchy_b"].any()
    s_np, st_np, _ = _frame()
    n = len(s_np)
    s, st = torch.from_numpy(s_np).cuda(), torch.from_numpy(st_np.view(np.int32)).cuda()
    lam = torch.full((n,), float(LAMBDA_D32), device="cuda")
    rays = cam.create_rays(s, wavelengths=lam, rng_states=st)["rays"]
    plain = cam.ray_differentials(s, rays, rng_states=st)
    d12 = cam.ray_differentials(s, rays, rng_states=st, wavelengths=lam)
    d18, ch = cam.ray_differentials(s, rays, rng_states=st, wavelengths=lam, chromatic=True)
    assert torch.equal(plain.view(torch.int32), d12.view(torch.int32))
    assert torch.equal(d12.view(torch.int32), d18.view(torch.int32))
    live = (rays[:, 6] != 0).cpu().numpy()
    assert live.sum() >= 4096
    assert bool((ch.view(torch.int32) & 0x7FFFFFFF).any()) and not _bits(ch.cpu().numpy()[~live]).any()
    lam2_np = bs.mixed_wavelengths(n)
    lam2 = torch.from_numpy(lam2_np).cuda()
    rays2 = cam.create_rays(s, wavelengths=lam2, rng_states=st)["rays"]
    a12 = cam.ray_differentials(s, rays2, rng_states=st, wavelengths=lam2)
    a18, ach = cam.ray_differentials(s, rays2, rng_states=st, wavelengths=lam2, chromatic=True)
    b18, bch = cam.ray_differentials(s, rays2, rng_states=st, wavelengths=lam2, chromatic=True)
    assert torch.equal(a12.view(torch.int32), a18.view(torch.int32))
    assert torch.equal(a18.view(torch.int32), b18.view(torch.int32)) and torch.equal(ach.view(torch.int32), bch.view(torch.int32))
    c18, cch = cam.ray_differentials(s, rays2, dsx=0.5, dsy=-0.25, rng_states=st, wavelengths=lam2, chromatic=True)
    assert torch.equal(cch.view(torch.int32), ach.view(torch.int32))
    a, c, r2 = a18.cpu().numpy(), c18.cpu().numpy(), rays2.cpu().numpy()
    live2 = r2[:, 6] != 0
    good = bs.valid(lam2_np)
    assert not live2[~good].any() and (r2[~good, 7].view(np.uint32) == 0x80).all() and live2.sum() >= 2048
    assert not _bits(a[~live2]).any() and not _bits(ach.cpu().numpy()[~live2]).any()
    assert (_bits(a[live2]) != 0).any(1).all()
    assert np.array_equal(c[live2][:, np.r_[0:3, 6:9]], (a[live2][:, np.r_[0:3, 6:9]] * F32(0.5)).astype(F32))
    assert np.array_equal(c[live2][:, np.r_[3:6, 9:12]], (a[live2][:, np.r_[3:6, 9:12]] * F32(-0.25)).astype(F32))
    assert not torch.equal(a12.view(torch.int32), d12.view(torch.int32))   # the wavelengths changed something
    cam.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_mode_independent_and_split_launches(gpu, name):
    """A STRICT and a FAST camera agree bit for bit wherever their records' weight and flag words agree: on at least 0.99 of the rows
    where FAST has a kernel of its own, on every row where it runs STRICT's.  Prefixes of 1, 63, 64 and 65 rays and a split at
    [0, 1, 64, 5037, n] with ray_index_base moved along equal the one launch; on the lenses of the most and the fewest interfaces so
    does the set tiled to 2048 x 256 + 65 rays (samples, streams and wavelengths tiled alike)."""
    import torch
    s, st, _ = _frame()
    n = len(s)
    lam = bs.mixed_wavelengths(n)
    a, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    b, _ = mc.camera(name, device=0, precision=PRECISION_FAST)
    ra, da, ca = _run(a, s, lam, base=1000)      # the streams the library derives from (seed, ray index)
    rb, db, cb = _run(b, s, lam, base=1000)
    same = (_bits(ra[:, 7]) == _bits(rb[:, 7])) & (_bits(ra[:, 6]) == _bits(rb[:, 6]))
    print("%-10s fastRunsStrict %s, records agree on %.5f of the rows" % (name, bool(b.info()["fastRunsStrict"]), same.mean()))
    assert same.all() if b.info()["fastRunsStrict"] else same.mean() >= 0.99
    assert np.array_equal(_bits(da[same]), _bits(db[same])) and np.array_equal(_bits(ca[same]), _bits(cb[same]))
    b.close()
    ts, tl, tr = torch.from_numpy(s).cuda(), torch.from_numpy(lam).cuda(), torch.from_numpy(ra).cuda()

    def part(lo, hi):
        d, c = a.ray_differentials(ts[lo:hi].contiguous(), tr[lo:hi].contiguous(), ray_index_base=1000 + lo,
                                   wavelengths=tl[lo:hi].contiguous(), chromatic=True)
        return d.cpu().numpy(), c.cpu().numpy()
    for m in PREFIXES:
        d, c = part(0, m)
        assert np.array_equal(_bits(d), _bits(da[:m])) and np.array_equal(_bits(c), _bits(ca[:m])), m
    parts = [part(lo, hi) for lo, hi in zip(SPLIT, SPLIT[1:] + [n])]
    assert np.array_equal(_bits(np.concatenate([d for d, _ in parts])), _bits(da))
    assert np.array_equal(_bits(np.concatenate([c for _, c in parts])), _bits(ca))
    if name in mc.LARGE_BATCH:
        reps = -(-BIG // n)
        big_s, big_l = np.tile(s, (reps, 1))[:BIG].copy(), np.tile(lam, reps)[:BIG].copy()
        big_st = np.tile(ray_rng_states(n, seed=1, ray_index_base=1000), (reps, 1))[:BIG].copy()
        rr, dd, cc = _run(a, big_s, big_l, states=big_st)
        assert np.array_equal(_bits(rr), np.tile(_bits(ra), (reps, 1))[:BIG])
        assert np.array_equal(_bits(dd), np.tile(_bits(da), (reps, 1))[:BIG]) and np.array_equal(_bits(cc), np.tile(_bits(ca), (reps, 1))[:BIG])
    a.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_zeros(gpu, name):
    """weight-0 rows, the forward call's rejected rows (flags 0x80) and live records given an invalid wavelength HERE -- one in each
    position of BAD inside one wave, and one whole wave -- get +0.0 in all 18 floats, and so does a wave whose weights are all set to
    0; their live neighbours in the same wave are unchanged"""
    import torch
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    s_np, st_np, lam_np = _frame()
    n = len(s_np)
    fwd = lam_np.copy()
    fwd_bad = np.arange(len(BAD)) * 9 + 130          # rejected by the forward call, mixed into waves 2 and 3
    fwd[fwd_bad] = BAD
    s, st, tf = torch.from_numpy(s_np).cuda(), torch.from_numpy(st_np.view(np.int32)).cuda(), torch.from_numpy(fwd).cuda()
    rays = cam.create_rays(s, wavelengths=tf, rng_states=st)["rays"]
    r = rays.cpu().numpy()
    assert (r[fwd_bad, 7].view(np.uint32) == 0x80).all()
    ref_d, ref_c = [x.cpu().numpy() for x in cam.ray_differentials(s, rays, rng_states=st, wavelengths=tf, chromatic=True)]
    assert not _bits(ref_d[fwd_bad]).any() and not _bits(ref_c[fwd_bad]).any()
    dead = r[:, 6] == 0
    assert not _bits(ref_d[dead]).any() and not _bits(ref_c[dead]).any()
    assert (_bits(ref_d[~dead]) != 0).any(1).all()
    # invalid wavelengths here on live records: one in each position of BAD within one wave, and the whole of another
    wm = _wave_with(~dead, len(BAD) + 1)
    ww = _wave_with(~dead, 1, after=wm)
    wz = _wave_with(~dead, 1, after=ww)
    mixed = np.flatnonzero(~dead[64 * wm:64 * wm + 64])[:len(BAD)] + 64 * wm
    here = lam_np.copy()
    here[mixed] = BAD
    here[64 * ww:64 * ww + 64] = np.resize(BAD, 64)
    here[fwd_bad] = fwd[fwd_bad]
    got_d, got_c = [x.cpu().numpy() for x in cam.ray_differentials(s, rays, rng_states=st, wavelengths=torch.from_numpy(here).cuda(), chromatic=True)]
    zero = np.zeros(n, bool)
    zero[mixed] = True
    zero[64 * ww:64 * ww + 64] = True
    assert not _bits(got_d[zero]).any() and not _bits(got_c[zero]).any()
    assert np.array_equal(_bits(got_d[~zero]), _bits(ref_d[~zero])) and np.array_equal(_bits(got_c[~zero]), _bits(ref_c[~zero]))
    assert (~dead & ~zero)[64 * wm:64 * wm + 64].any() and (_bits(ref_d[mixed]) != 0).any(1).all()
    # a wave whose records are all dead: every weight set to 0
    r2 = rays.clone()
    r2[64 * wz:64 * wz + 64, 6] = 0.0
    d2, c2 = [x.cpu().numpy() for x in cam.ray_differentials(s, r2, rng_states=st, wavelengths=tf, chromatic=True)]
    assert not _bits(d2[64 * wz:64 * wz + 64]).any() and not _bits(c2[64 * wz:64 * wz + 64]).any()
    keep = np.r_[0:64 * wz, 64 * wz + 64:n]
    assert np.array_equal(_bits(d2[keep]), _bits(ref_d[keep])) and np.array_equal(_bits(c2[keep]), _bits(ref_c[keep]))
    cam.close()


def test_five_column_lens_is_four_columns_and_its_v_column(gpu):
    """tessar-5 carries its V-numbers in a fifth column: the same prescription loaded as four columns plus set_abbe_numbers with that
    column gives the same dispersion table, records and differentials, bit for bit"""
    rows = rows_of(mc.LENSES["tessar-5"].text)
    assert all(len(r) == 5 for r in rows) and mc.LENSES["tessar-5"].abbe is None
    four = MachineLens("".join("\t".join("%.6g" % v for v in (r[0], r[1], r[2], r[4])) + "\n" for r in rows), np.array([r[3] for r in rows], F32))
    a, p = mc.camera("tessar-5", device=0, precision=PRECISION_STRICT)
    b = ZoicCamera(device=0)
    four.load(b)
    b.set_precision(PRECISION_STRICT)
    b.update(**p)
    da, db = a.dispersion(), b.dispersion()
    assert da["cauchy_b"].any() and len(set(da["cauchy_b"][da["cauchy_b"] != 0].tolist())) >= 3   # distinct V-numbers
    assert np.array_equal(_bits(da["cauchy_b"]), _bits(db["cauchy_b"])) and np.array_equal(_bits(da["ior_d"]), _bits(db["ior_d"]))
    s, st, lam = _frame()
    ra, xa, ca = _run(a, s, lam, states=st)
    rb, xb, cb = _run(b, s, lam, states=st)
    assert np.array_equal(_bits(ra), _bits(rb)) and np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ca), _bits(cb))
    assert (ra[:, 6] != 0).sum() >= 4096 and (_bits(ca[ra[:, 6] != 0]) != 0).any(1).all()
    a.close()
    b.close()


# ---- D: round trip with the spectral Jacobian ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCURACY)
def test_round_trip_with_the_spectral_jacobian(gpu, oracle_lib, name):
    """FAST camera, test_traceback_jacobian_gpu's frame (64 x 36 x 2), wavelengths uniform in [400, 700] nm.  T_lambda = [dOdx dOdy;
    dDdx dDdy] of ray_differentials(..., wavelengths=lam), J_lambda of trace_back_jacobian(fwd, wavelengths=lam): with the lens point
    and the wavelength held fixed every member of that ray family traces back to its own sample, so J_lambda T_lambda = I -- three
    kernels written independently (spectral forward, spectral differentials, spectral Jacobian).  Rays kept as
    test_round_trip_against_the_forward_differentials keeps them (weight > 0, traced back, off TraceBack.edge by the f64 trace at the
    ray's wavelength rounded to whole nanometres, T != 0), in the spectral AND in the d-line run; about 512 of them.  Yardstick: the
    d-line |J T - I|_max of the same rays in the same run (no wavelengths given to either call; both kernels are held to finite
    differences there).  The spectral residual may be 2 x that, median and 99th percentile: the margin the backward corpus gives a
    spectral round trip over its d-line one."""
    import torch
    cam, p = mc.camera(name, device=0, precision=PRECISION_FAST)
    info, disp = cam.info(), cam.dispersion()
    n = jr.N
    smp = torch.from_numpy(synthetic_samples(n, jr.W, jr.H, jr.SPP)).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(n).view(np.int32)).to("cuda:0")
    lam_h = np.random.default_rng(23).uniform(400.0, 700.0, n).astype(F32)
    lam = torch.from_numpy(lam_h).to("cuda:0")
    Tb = bs.SpectralTraceBack(info, p, disp)

    def run(w):
        kw = {} if w is None else dict(wavelengths=w)
        fwd = cam.create_rays(smp, rng_states=st, **kw)
        diffs = cam.ray_differentials(smp, fwd, rng_states=st, **kw)
        scr, fl, jac = cam.trace_back_jacobian(fwd, **kw)
        torch.cuda.synchronize()
        rec, diffs, jac, fl = fwd["rays"].cpu().numpy(), diffs.cpu().numpy().astype(np.float64), jac.cpu().numpy().astype(np.float64), fl.cpu().numpy()
        T = np.concatenate([np.stack([diffs[:, 0:3], diffs[:, 3:6]], 2), np.stack([diffs[:, 6:9], diffs[:, 9:12]], 2)], 1)   # (n,6,2)
        ref = Tb.trace(rec[:, 0:3], rec[:, 3:6]) if w is None else Tb.trace_at(rec[:, 0:3], rec[:, 3:6], np.round(lam_h))
        keep = (rec[:, 6] > 0) & ref["traced"] & ~Tb.edge(ref) & ((fl & 1) == 1) & (np.abs(T).max((1, 2)) > 0)
        assert keep.sum() > 0.5 * (rec[:, 6] > 0).sum()
        return keep, jac, T
    keep0, jac0, T0 = run(None)
    keep1, jac1, T1 = run(lam)
    keep = keep0 & keep1
    pick = np.flatnonzero(keep)[:: max(1, keep.sum() // 512)][:512]
    assert len(pick) >= 384, len(pick)
    r0 = jr.residual(jac0[pick], T0[pick])
    r1 = jr.residual(jac1[pick], T1[pick])
    print("%-10s %d rays; |J T - I| spectral median %.3g p99 %.3g; d-line median %.3g p99 %.3g; ratios %.2f / %.2f" % (
        name, len(pick), np.median(r1), np.percentile(r1, 99), np.median(r0), np.percentile(r0, 99), np.median(r1) / np.median(r0),
        np.percentile(r1, 99) / np.percentile(r0, 99)))
    assert np.median(r1) <= 2.0 * np.median(r0), (np.median(r1), np.median(r0))
    assert np.percentile(r1, 99) <= 2.0 * np.percentile(r0, 99), (np.percentile(r1, 99), np.percentile(r0, 99))
    cam.close()

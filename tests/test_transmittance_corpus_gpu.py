"""Fresnel transmittance on the MI355X (zoic_ray_transmittance_device) over the pinned corpus of machine-made lenses and plates-32, the
lens that fills the tables (tests/lens_losses_corpus.py), after tests/test_transmittance_corpus_cpu.py, which holds the host build of
csrc/transmittance.hpp to the f64 restatement on the same lenses:

  A  the kernel gives the host build bit for bit, bare and with a film wherever the media differ, STRICT, on reference_rows of the
     live records of the frame: k = 1 on the spectral records, k = 4 on hero records whose hero wavelength is the frame's and whose
     three companions rotate through spectral_ref.WAVES (their start is the hero's accepted try);
  B  the identities of the call on the whole frame (41 472 rows), bit for bit: column 0 of the k = 4 call against the k = 1 call (the
     store through the LDS transpose against the direct store), the d-line form, two runs, prefixes, split launches, STRICT against
     FAST, and on the lenses of the most and the fewest interfaces and on plates-32 the frame tiled to 2048 x 256 + 65 rows at k = 1;
  C  zeros: forward-rejected rows, weight-0 rows and rejected wavelengths, single in a wave and as a whole wave, give +0.0 and leave
     their live neighbours alone.

Measured on the MI355X (every comparison is exact, so the figures are the sizes of what was compared).  A, per lens: rows, the
kernel's median T at k = 1 bare / with the film, and the companions of the k = 4 records that were lost (weight 0, T = +0.0):

    lens       rows  T median bare / film  companions lost
    triplet-4  3753  0.762 / 0.974            25 of 11 259
    fisheye-5  3903  0.529 / 0.890            45 of 11 709
    mori-6     4001  0.470 / 0.939            56 of 12 003
    double-3   3858  0.592 / 0.850            89 of 11 574
    tessar-5   3802  0.677 / 0.863            17 of 11 406
    petzval-2  3656  0.741 / 0.905            34 of 10 968
    mori-4     3911  0.676 / 0.851             3 of 11 733
    rear-9     3782  0.678 / 0.921         1 169 of 11 346
    rear-12    3871  0.678 / 0.922           625 of 11 613
    petzval-5  3655  0.664 / 0.851           319 of 10 965
    plates-32  3876  0.207 / 0.697            67 of 11 628

No word differs on any lens in A, B or C.  B: the STRICT and the FAST camera's records agree on every row of every lens (petzval-5
runs STRICT's kernels), and no live record of a FAST camera has T == 0: 0 of 25 450 (triplet-4), 41 472 (fisheye-5), 32 560 (mori-6),
41 472 (double-3), 22 629 (tessar-5), 16 412 (petzval-2), 18 464 (mori-4), 23 315 (rear-9), 38 155 (rear-12), 11 169 (petzval-5) and
41 472 (plates-32) live records of this frame.  Nothing is asserted on that share.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT
from zoic_amd.workloads import ray_rng_states

import backward_spectral_ref as bs
import lens_losses_corpus as lc
import machine_lens_corpus as mc
import host_drivers
from device_cases import bits_f32 as _bits
from differentials_spectral_corpus import frame, wave_with as _wave_with
from host_drivers import run_transmittance as run_driver
from lens_losses_corpus import (BIG, SPLIT, device_camera as _camera, device_inputs as _inputs, device_launch as _launch, device_starts as _starts,
                                same_words as _same, take as _take)
from machine_lens_corpus import PREFIXES
from spectral_ref import BAD, LAMBDA_D32, WAVES

pytestmark = pytest.mark.gpu

F32 = np.float32
K = 4


@pytest.fixture(scope="module")
def driver():
    return host_drivers.transmittance()


def _hero_wavelengths(rows):
    """(len(rows), K) wavelengths: the frame's as the hero, three companions rotated through WAVES"""
    lam = np.zeros((len(rows), K), F32)
    lam[:, 0] = frame()[2][rows]
    for j in range(1, K):
        lam[:, j] = WAVES[(np.asarray(rows) + j) % len(WAVES)]
    return lam


# ---- A: host == device bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_kernel_equals_the_host_build(gpu, oracle_lib, driver, name, coated):
    """STRICT, reference_rows of the live records (at most 4096), the starts from the records' tries.  k = 1: the spectral records.
    k = 4: create_rays_hero's records of the same samples and streams, whose column 0 is the spectral record; every column's T is the
    host build's from the hero's start at the column's wavelength where the column's record has weight.  0 < T < 1 on every live
    column, +0.0 elsewhere."""
    import torch
    T, S = lc.tables(name), _starts(oracle_lib, name)
    rows = S["rows"]
    film = T["film"] if coated else None
    cam = _camera(name, coated=coated)
    ts, tl, tst, tr = _take(rows, _launch(name)[rows])
    got1 = cam.transmittance(ts, tr, wavelengths=tl, rng_states=tst)
    assert tuple(got1.shape) == (len(rows),) and got1.dtype == torch.float32
    g1 = got1.cpu().numpy()
    want1 = run_driver(driver, T["surf"], T["disp"], S["lam"], S["o"], S["d"], film, T["housing2"])
    differ = np.flatnonzero(_bits(g1) != _bits(want1))
    assert len(differ) == 0, (name, len(differ), differ[:8].tolist())
    assert (g1 > 0).all() and (g1 < 1).all() and len(rows) >= 2048
    # k = 4
    lam4 = _hero_wavelengths(rows)
    tl4 = torch.from_numpy(lam4).cuda()
    hero = cam.create_rays_hero(ts, tl4, rng_states=tst)["rays"]
    assert _same(hero[:, 0], tr)                                      # the hero's record is the spectral record: the same try
    got4 = cam.transmittance(ts, hero, wavelengths=tl4, rng_states=tst)
    torch.cuda.synchronize()
    assert tuple(got4.shape) == (len(rows), K)
    g4, w = got4.cpu().numpy(), hero[:, :, 6].cpu().numpy()
    want4 = np.zeros((len(rows), K), F32)
    for j in range(K):
        live = np.flatnonzero(w[:, j] != 0)
        want4[live, j] = run_driver(driver, T["surf"], T["disp"], lam4[live, j], S["o"][live], S["d"][live], film, T["housing2"])
    differ = np.argwhere(_bits(g4) != _bits(want4))
    assert len(differ) == 0, (name, len(differ), differ[:8].tolist())
    assert (g4[w != 0] > 0).all() and (g4 < 1).all() and not _bits(g4[w == 0]).any()
    lost = int((w[:, 1:] == 0).sum())
    print("%-10s %-5s rows %4d  T median %.3f (k = 1)  companions lost %d of %d" % (name, "film" if coated else "bare", len(rows), np.median(g1),
                                                                                  lost, 3 * len(rows)))
    assert (w[:, 1:] != 0).sum() >= 3 * 2048
    cam.close()


# ---- B: identities on the whole frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_column_and_d_line_identities(gpu, name):
    """the whole frame, with the film, the library's own streams at a ray_index_base: column 0 of the k = 4 call is the k = 1 call on
    rays[:, 0] and lam[:, 0] (the k > 1 kernel stores through an LDS transpose, the k = 1 kernel directly); two runs are equal; the
    d-line form on create_rays' records equals the call given 587.5618 nm per sample, as (n,) and as (n, 1)"""
    import torch
    cam = _camera(name, coated=True)
    ts, _, tl = _inputs()
    n, base = len(ts), 1000
    lam4 = torch.from_numpy(_hero_wavelengths(np.arange(n))).cuda()
    hero = cam.create_rays_hero(ts, lam4, ray_index_base=base)["rays"]
    t4 = cam.transmittance(ts, hero, wavelengths=lam4, ray_index_base=base)
    t1 = cam.transmittance(ts, hero[:, 0].contiguous(), wavelengths=lam4[:, 0].contiguous(), ray_index_base=base)
    assert tuple(t4.shape) == (n, K) and tuple(t1.shape) == (n,)
    assert _same(t4[:, 0], t1)
    assert _same(cam.transmittance(ts, hero, wavelengths=lam4, ray_index_base=base), t4)
    live = hero[:, :, 6] != 0
    assert bool(((t4 > 0) == live).all()) and int(live[:, 0].sum()) >= 4096 and int(live[:, 1:].sum()) >= 3 * 4096
    rays0 = cam.create_rays(ts, ray_index_base=base)["rays"]
    d = torch.full((n,), float(LAMBDA_D32), device="cuda")
    a = cam.transmittance(ts, rays0, ray_index_base=base)
    b = cam.transmittance(ts, rays0, wavelengths=d, ray_index_base=base)
    c = cam.transmittance(ts, rays0.view(n, 1, 8), wavelengths=d.view(n, 1), ray_index_base=base)
    assert _same(a, b) and _same(a, c.view(n)) and bool(((a > 0) == (rays0[:, 6] != 0)).all())
    torch.cuda.synchronize()
    cam.close()


@pytest.mark.parametrize("name", lc.NAMES)
def test_mode_independent_and_split_launches(gpu, name):
    """A STRICT and a FAST camera agree bit for bit wherever their records' weight and flag words agree: on at least 0.99 of the rows
    where FAST has a kernel of its own, on every row where it runs STRICT's (the shares of the spectral-differentials corpus test).
    Prefixes of 1, 63, 64 and 65 rows and a split at [0, 1, 64, 5037, n] with ray_index_base moved along equal the one launch; on the
    lenses of the most and the fewest interfaces and on plates-32 so does the frame tiled to 2048 x 256 + 65 rows at k = 1 (samples,
    streams and wavelengths tiled alike).  Printed, not asserted: the share of a FAST camera's live records with T == 0, starts FAST
    accepted that the STRICT replay of this pass clips."""
    import torch
    ts, _, tl = _inputs()
    n, base = len(ts), 1000
    a = _camera(name, coated=True)
    b = _camera(name, precision=PRECISION_FAST, coated=True)
    ra = a.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    rb = b.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    ta = a.transmittance(ts, ra, wavelengths=tl, ray_index_base=base)
    tb = b.transmittance(ts, rb, wavelengths=tl, ray_index_base=base)
    same = (ra[:, 6:8].contiguous().view(torch.int32) == rb[:, 6:8].contiguous().view(torch.int32)).all(1)
    share = float(same.float().mean())
    live_b = rb[:, 6] != 0
    print("%-10s fastRunsStrict %s, records agree on %.5f of the rows; FAST live records with T == 0: %d of %d" % (
        name, bool(b.info()["fastRunsStrict"]), share, int(((tb == 0) & live_b).sum()), int(live_b.sum())))
    assert share == 1.0 if b.info()["fastRunsStrict"] else share >= 0.99
    assert _same(ta[same], tb[same])
    assert bool(((ta > 0) == (ra[:, 6] != 0)).all())                  # STRICT: every live record has a path
    b.close()

    def part(lo, hi):
        return a.transmittance(ts[lo:hi].contiguous(), ra[lo:hi].contiguous(), wavelengths=tl[lo:hi].contiguous(), ray_index_base=base + lo)
    for m in PREFIXES:
        assert _same(part(0, m), ta[:m]), m
    assert _same(torch.cat([part(lo, hi) for lo, hi in zip(SPLIT, SPLIT[1:] + [n])]), ta)
    if name in mc.LARGE_BATCH or name == lc.PLATES:
        reps = -(-BIG // n)
        st = torch.from_numpy(ray_rng_states(n, seed=1, ray_index_base=base).view(np.int32)).cuda()
        big_s, big_l, big_st = ts.repeat(reps, 1)[:BIG].contiguous(), tl.repeat(reps)[:BIG].contiguous(), st.repeat(reps, 1)[:BIG].contiguous()
        rr = a.create_rays(big_s, wavelengths=big_l, rng_states=big_st)["rays"]
        assert _same(rr, ra.repeat(reps, 1)[:BIG])
        tt = a.transmittance(big_s, rr, wavelengths=big_l, rng_states=big_st)
        assert tuple(tt.shape) == (BIG,) and _same(tt, ta.repeat(reps)[:BIG])
    torch.cuda.synchronize()
    a.close()


# ---- C: zeros -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_zeros(gpu, name):
    """weight-0 rows, the forward call's rejected rows (flags 0x80) and live records given an invalid wavelength HERE -- one in each
    position of BAD inside one wave, and one whole wave -- get +0.0, and so does a wave whose weights are all set to 0; their live
    neighbours in the same wave are unchanged (test_differentials_spectral_corpus_gpu.test_zeros on this pass)"""
    import torch
    cam = _camera(name, coated=True)
    ts, tst, _ = _inputs()
    lam_np = np.array(frame()[2])
    n = len(lam_np)
    fwd = lam_np.copy()
    fwd_bad = np.arange(len(BAD)) * 9 + 130          # rejected by the forward call, mixed into waves 2 and 3
    fwd[fwd_bad] = BAD
    tf = torch.from_numpy(fwd).cuda()
    rays = cam.create_rays(ts, wavelengths=tf, rng_states=tst)["rays"]
    r = rays.cpu().numpy()
    assert (_bits(r[fwd_bad, 7]) == 0x80).all()
    ref = cam.transmittance(ts, rays, wavelengths=tf, rng_states=tst).cpu().numpy()
    dead = r[:, 6] == 0
    assert not _bits(ref[fwd_bad]).any() and not _bits(ref[dead]).any() and (ref[~dead] > 0).all() and dead.sum() >= len(BAD)
    wm = _wave_with(~dead, len(BAD) + 1)
    ww = _wave_with(~dead, 1, after=wm)
    wz = _wave_with(~dead, 1, after=ww)
    mixed = np.flatnonzero(~dead[64 * wm:64 * wm + 64])[:len(BAD)] + 64 * wm
    here = lam_np.copy()
    here[mixed] = BAD
    here[64 * ww:64 * ww + 64] = np.resize(BAD, 64)
    here[fwd_bad] = fwd[fwd_bad]
    got = cam.transmittance(ts, rays, wavelengths=torch.from_numpy(here).cuda(), rng_states=tst).cpu().numpy()
    zero = np.zeros(n, bool)
    zero[mixed] = True
    zero[64 * ww:64 * ww + 64] = True
    assert not _bits(got[zero]).any() and np.array_equal(_bits(got[~zero]), _bits(ref[~zero]))
    assert (~dead & ~zero)[64 * wm:64 * wm + 64].any() and (ref[mixed] > 0).all() and bs.valid(here[~zero & ~dead]).all()
    r2 = rays.clone()
    r2[64 * wz:64 * wz + 64, 6] = 0.0
    got2 = cam.transmittance(ts, r2, wavelengths=tf, rng_states=tst).cpu().numpy()
    assert not _bits(got2[64 * wz:64 * wz + 64]).any() and (ref[64 * wz:64 * wz + 64] > 0).any()
    keep = np.r_[0:64 * wz, 64 * wz + 64:n]
    assert np.array_equal(_bits(got2[keep]), _bits(ref[keep]))
    cam.close()

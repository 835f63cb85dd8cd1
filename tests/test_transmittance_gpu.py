"""Fresnel transmittance of traced rays on the MI355X (zoic_ray_transmittance_device): the kernel gives the host build of
csrc/transmittance.hpp bit for bit on all n x k columns -- the starts from the CPU reference of the hero call (tests/hero_ref.py) or
from differentials_ref.kolb_start, the lens's own clip limits in the host build -- with and without coatings, on STRICT and FAST
cameras; the columns without a ray or without a wavelength get +0.0; the d-line form, the other lens models, split launches and the
error codes are the header's; the records and the counters are left alone.

Sizes: 1, 63, 65 and 4096 samples at k = 1, 3 and 8, and 524 353 = 2048 x 256 + 65 samples at k = 1, the first size at which the
grid-stride loop takes a second turn and that turn ends in a partial wave."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.camera import ZoicError
from zoic_amd.workloads import ray_rng_states

import differentials_ref as dref
import hero_cases as hr
import host_drivers
from device_cases import BIG, bits_f32 as _bits, camera as _camera, oracle as _oracle, params as _params, samples as _samples
from hero_cases import LOSS_CAMERAS as CAMERAS, cycled as _cycled, loss_reference as _reference
from host_drivers import run_transmittance as run_driver
from spectral_ref import BAD, LAMBDA_D32, WAVES
from transmittance_cases import coat as _coat, expected as _expected, tables as _tables
from transmittance_ref import FILM_INDEX, FILM_LAMBDA0

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 4096
SIZES = [1, 63, 65, N]


@pytest.fixture(scope="module")
def driver():
    return host_drivers.transmittance()


def _forward(cam, s, lam, st, base=0):
    import torch
    ts, tl = torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(lam)).cuda()
    tst = None if st is None else torch.from_numpy(np.array(st).view(np.int32)).cuda()
    rays = cam.create_rays_hero(ts, tl, rng_states=tst, ray_index_base=base)["rays"]
    return ts, tl, tst, rays


# ---- host == device bits, n x k -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [PRECISION_STRICT, PRECISION_FAST], ids=["strict", "fast"])
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_kernel_equals_the_host_build(gpu, oracle_lib, driver, cfg, k, coated, precision):
    """every column of n = 1, 63, 65 and 4096 samples.  STRICT records are the reference's, so every row is compared; a FAST record may
    end at another try than the reference's (then its start is not the recorded one): those rows, fewer than 1 in 1000, are left to
    the STRICT case"""
    import torch
    name = CAMERAS[cfg]
    s, lam, st, words, starts = _reference(oracle_lib, name, k)
    cam = _coat(hr.spec(name).camera(precision=precision), name, coated)
    seen_live = seen_dead = 0
    for n in SIZES:
        ts, tl, tst, rays = _forward(cam, s[:n], lam[:n], st[:n])
        got = cam.transmittance(ts, rays, wavelengths=tl, rng_states=tst)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (n, k) and got.dtype == torch.float32
        r = rays.cpu().numpy()
        w = r[:, :, 6]
        known = r[:, 0, 7].view(np.uint32) == words[:n, 0, 7]           # the hero's flag word: its try count among it
        if precision == PRECISION_STRICT:
            assert hr.same_words(r.view(np.uint32), words[:n]).all()
        else:
            assert known.mean() >= 0.999 or n < 1000
        want = _expected(driver, name, coated, starts[:n], lam[:n], w)
        g = got.cpu().numpy()
        assert np.array_equal(_bits(g[known]), _bits(want[known])), (n, np.argwhere(_bits(g) != _bits(want))[:8].tolist())
        live = (w != 0) & hr.valid(lam[:n])
        assert (g < 1).all() and not _bits(g[~live]).any()
        if precision == PRECISION_STRICT:      # T > 0 iff the path passes, and a STRICT record's does
            assert (g[live] > 0).all()
        seen_live += int(live[known].sum())
        seen_dead += int((~live[known]).sum())
    assert seen_live >= 1000 * k and seen_dead >= 100
    cam.close()


def test_second_grid_turn_and_ragged_wave(gpu, oracle_lib, driver):
    """n = 2048 x 256 + 65, k = 1, the library's own retry streams at a ray_index_base: all rows against the two-pass identity (the
    same bits from launches of the two halves), 16 Ki random rows and the last 129 against the host build from kolb_start"""
    import torch
    p = _params("C2")
    cam = _coat(_camera(p), "C2", True)
    base = 1000
    s = _samples(BIG, seed=7)
    lam = np.resize(WAVES, BIG).astype(F32)
    states = ray_rng_states(BIG, seed=1)           # seed 1, no base: the streams the library derives itself ...
    ts, tl = torch.from_numpy(s).cuda(), torch.from_numpy(lam).cuda()
    rays = cam.create_rays(ts, wavelengths=tl)["rays"]
    got = cam.transmittance(ts, rays, wavelengths=tl)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (BIG,)
    g, r = got.cpu().numpy(), rays.cpu().numpy()
    idx = np.unique(np.r_[np.random.RandomState(1).choice(BIG, 1 << 14, replace=False), BIG - 129:BIG])
    live = idx[r[idx, 6] != 0]
    tries = ((r[live, 7].view(np.uint32) >> 1) & 31).astype(np.int64)
    assert int((tries > 0).sum()) >= 200
    oc = _oracle(oracle_lib, p)
    o0, d0 = dref.kolb_start(oc, p, s[live], tries, states[live], oracle_lib)
    disp, surf, h2, film = _tables("C2")
    want = run_driver(driver, surf, disp, lam[live], o0, d0, film, h2)
    assert np.array_equal(_bits(g[live]), _bits(want))
    assert (g[r[:, 6] != 0] > 0).all() and not _bits(g[r[:, 6] == 0]).any()
    assert (r[BIG - 65:, 6] != 0).any()
    # ... and two halves at their ray_index_base, the second starting in the middle of a wave
    rays_b = cam.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    whole = cam.transmittance(ts, rays_b, wavelengths=tl, ray_index_base=base)
    cut = BIG // 2 + 7
    parts = [cam.transmittance(ts[lo:hi].contiguous(), rays_b[lo:hi].contiguous(), wavelengths=tl[lo:hi].contiguous(), ray_index_base=base + lo)
             for lo, hi in ((0, cut), (cut, BIG))]
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32))
    cam.close()


# ---- rows that get +0.0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
def test_columns_that_get_zero(gpu, oracle_lib, driver, k):
    """lost companions, rejected columns (BAD wavelengths in the forward call: a hero's rejects its row), heroes of weight 0, and BAD
    wavelengths HERE on live records -- single lanes, a hero's column alone, a whole wave -- all in one batch, every column compared
    with the host build; then a wave whose records are all dead"""
    import torch
    name = "C2"
    fwd = _cycled(N, k).copy()
    hero_bad = np.arange(len(BAD)) * 9 + 130                 # mixed into waves 2 and 3
    fwd[hero_bad, 0] = BAD
    if k > 1:
        comp_bad = np.arange(len(BAD)) * 11 + 260
        fwd[comp_bad, 1 + np.arange(len(BAD)) % (k - 1)] = BAD
    s, lam, st, words, starts = _reference(oracle_lib, name, k, fwd, "zeros")
    cam = _coat(hr.spec(name).camera(), name, True)
    ts, tl, tst, rays = _forward(cam, s, lam, st)
    r = rays.cpu().numpy()
    assert hr.same_words(r.view(np.uint32), words).all()
    w, flags = r[:, :, 6], r[:, :, 7].view(np.uint32)
    assert (flags[hero_bad] == hr.REJECTED).all() and (w[:, 0] == 0).sum() >= 100
    if k > 1:
        lost = ((flags[:, 1:] & hr.LOST) != 0) & (w[:, :1] != 0)
        assert lost.sum() >= 8 and (w[:, 1:][lost] == 0).all(), int(lost.sum())
        assert (flags[comp_bad, 1 + np.arange(len(BAD)) % (k - 1)] == hr.REJECTED).all()
    here = lam.copy()
    live_rows = np.nonzero((w != 0).all(1))[0]
    mixed = live_rows[(live_rows >= 320) & (live_rows < 384)][:len(BAD)]
    assert len(mixed) == len(BAD)
    here[mixed, 0] = BAD                                      # the hero's column alone: its companions keep their start
    if k > 1:
        here[mixed[::-1], k - 1] = BAD[:len(mixed)]
    here[448:512] = np.resize(BAD, (64, k))                   # a whole wave
    assert (w[448:512] != 0).any()
    got = cam.transmittance(ts, rays, wavelengths=torch.from_numpy(here).cuda(), rng_states=tst).cpu().numpy()
    want = _expected(driver, name, True, starts, here, w)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8].tolist()
    assert not _bits(got[448:512]).any() and not _bits(got[mixed, 0]).any() and not _bits(got[w == 0]).any()
    if k > 1:
        assert (got[mixed[1:-1], 1:k - 1] > 0).all() or k < 3
    ref = cam.transmittance(ts, rays, wavelengths=tl, rng_states=tst).cpu().numpy()
    assert (ref[mixed, 0] > 0).all()
    # a wave whose records are all dead
    r2 = rays.clone()
    r2[64:128, :, 6] = 0.0
    got2 = cam.transmittance(ts, r2, wavelengths=tl, rng_states=tst).cpu().numpy()
    assert not _bits(got2[64:128]).any()
    keep = np.r_[0:64, 128:N]
    assert np.array_equal(_bits(got2[keep]), _bits(ref[keep])) and (ref[64:128] > 0).any()
    cam.close()


# ---- the d-line form, the other lens models -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_d_line_form(gpu, n):
    """NULL wavelengths on create_rays records == the k = 1 call at 587.5618, bit for bit; both as (n,) and as (n, 1)"""
    import torch
    cam = _coat(_camera(_params("C2")), "C2", True)
    s = torch.from_numpy(_samples(n, seed=11)).cuda()
    rays = cam.create_rays(s, ray_index_base=5)["rays"]
    lam = torch.full((n,), float(LAMBDA_D32), device="cuda")
    a = cam.transmittance(s, rays, ray_index_base=5)
    b = cam.transmittance(s, rays, wavelengths=lam, ray_index_base=5)
    c = cam.transmittance(s, rays.view(n, 1, 8), wavelengths=lam.view(n, 1), ray_index_base=5)
    assert tuple(a.shape) == (n,) and tuple(c.shape) == (n, 1)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32).view(n))
    live = rays[:, 6] != 0
    assert bool(((a > 0) == live).all()) and (n < 63 or bool(live.any()))
    # the spectral call's records at the d-line are create_rays' own: the same T from them
    rays_s = cam.create_rays(s, wavelengths=lam, ray_index_base=5)["rays"]
    assert torch.equal(cam.transmittance(s, rays_s, wavelengths=lam, ray_index_base=5).view(torch.int32), a.view(torch.int32))
    cam.close()


@pytest.mark.parametrize("over", [{}, dict(useDof=False), dict(opticalVignettingDistance=5.0)], ids=["C1", "C1-noDOF", "C1-vignet"])
def test_thin_lens_gives_ones_and_zeros(gpu, over):
    import torch
    cam = _camera(_params("C1", **over))
    n, k = 4096 + 65, 3
    s = torch.from_numpy(_samples(n, seed=19)).cuda()
    lam_np = _cycled(n, k)
    lam_np[np.arange(len(BAD)) * 97 + 5, 0] = BAD
    lam_np[np.arange(len(BAD)) * 89 + 9, 2] = BAD
    lam = torch.from_numpy(lam_np).cuda()
    rays = cam.create_rays_hero(s, lam)["rays"]
    here = lam_np.copy()
    here[np.arange(len(BAD)) * 83 + 2, 1] = BAD
    got = cam.transmittance(s, rays, wavelengths=torch.from_numpy(here).cuda()).cpu().numpy()
    w = rays[:, :, 6].cpu().numpy()
    want = ((w != 0) & hr.valid(here)).astype(F32)
    assert np.array_equal(_bits(got), _bits(want))
    assert (want == 1).any() and (want == 0).sum() >= 3 * len(BAD)
    r1 = cam.create_rays(s)["rays"]
    one = cam.transmittance(s, r1).cpu().numpy()
    assert np.array_equal(_bits(one), _bits((r1[:, 6].cpu().numpy() != 0).astype(F32)))
    cam.close()


def test_lens_model_none_gives_zeros(gpu):
    import torch
    cam = _camera(_params("C2"))
    s = torch.from_numpy(_samples(4096)).cuda()
    lam = torch.from_numpy(_cycled(4096, 3)).cuda()
    rays = cam.create_rays_hero(s, lam)["rays"]
    cam.update(**_params("C2", lensModel=2))
    out = torch.full((4096, 3), 7.0, device="cuda")
    got = cam.transmittance(s, rays, wavelengths=lam, out=out)
    torch.cuda.synchronize()
    assert got is out and not got.view(torch.int32).any()
    cam.close()


# ---- split launches, records untouched, coatings read at the call ----------------------------------------------------------------
def test_split_launches_and_records_untouched(gpu):
    """k = 3 on the camera without the exit-pupil LUT (half of its heroes retry: the streams matter): pieces with their ray_index_base
    give one launch's bits; the records, the inputs and the camera's counters are bitwise what they were; the film table is read at
    the call"""
    import torch
    name = "C2-nolut"
    cam = hr.spec(name).camera()
    n, k, base = N + 37, 3, 777
    s, lam = hr.samples(n, 5), _cycled(n, k)
    ts, tl, _, rays = _forward(cam, s, lam, None, base)
    before = cam.counters()
    keep = [t.clone() for t in (ts, tl, rays)]
    bare = cam.transmittance(ts, rays, wavelengths=tl, ray_index_base=base)
    cut = [0, 1, 64, 2000 + 37, n]
    parts = [cam.transmittance(ts[lo:hi].contiguous(), rays[lo:hi].contiguous(), wavelengths=tl[lo:hi].contiguous(), ray_index_base=base + lo)
             for lo, hi in zip(cut[:-1], cut[1:])]
    assert torch.equal(torch.cat(parts).view(torch.int32), bare.view(torch.int32))
    wrong = cam.transmittance(ts, rays, wavelengths=tl, ray_index_base=base + 1)       # another stream: other starts for the retried
    assert not torch.equal(wrong.view(torch.int32), bare.view(torch.int32))
    count = cam.info()["lensCount"]
    cam.set_coatings(np.full(count, FILM_INDEX, F32), FILM_LAMBDA0)
    film = cam.transmittance(ts, rays, wavelengths=tl, ray_index_base=base)
    live = bare > 0
    assert bool(live.any()) and bool((film[live] > bare[live]).all()) and torch.equal(film > 0, live)
    cam.set_coatings(None, None)
    assert torch.equal(cam.transmittance(ts, rays, wavelengths=tl, ray_index_base=base).view(torch.int32), bare.view(torch.int32))
    torch.cuda.synchronize()
    for a, b in zip(keep, (ts, tl, rays)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert cam.counters() == before
    assert ((rays[:, 0, 7].view(torch.int32) >> 1) & 31).gt(0).sum() >= 1000
    cam.close()


def test_error_codes(gpu):
    import torch
    lib = gpu
    OK, INVALID, NOT_UPDATED = 0, _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT"), _capi.STATUS_NAMES.index("ZOIC_ERR_NOT_UPDATED")
    cam = ZoicCamera(device=0)
    s = torch.zeros((64, 4), device="cuda")
    r = torch.zeros((64 * 2 + 1, 8), device="cuda")
    o = torch.zeros((64 * 2 + 1,), device="cuda")
    w = torch.full((64 * 2 + 1,), 500.0, device="cuda")
    st = C.c_void_p(0)
    f = lib.zoic_ray_transmittance_device
    S, R, O, W = s.data_ptr(), r.data_ptr(), o.data_ptr(), w.data_ptr()
    assert f(cam._h, 64, 1, S, W, None, 0, R, O, st) == NOT_UPDATED
    assert f(cam._h, 64, 0, S, W, None, 0, R, O, st) == INVALID        # k first
    cam.update(**_params("C2"))
    assert f(cam._h, 0, 1, None, None, None, 0, None, None, st) == OK
    assert f(cam._h, 0, 9, None, None, None, 0, None, None, st) == INVALID
    assert f(cam._h, 64, 1, S, W, None, 0, R, O, st) == OK
    assert f(cam._h, 64, 1, S, None, None, 0, R, O, st) == OK           # the d-line form
    assert f(cam._h, 64, 2, S, W, None, 0, R, O, st) == OK
    assert f(cam._h, 64, 2, S, W + 4, None, 0, R + 32, O + 4, st) == OK
    assert f(cam._h, 64, 2, S, None, None, 0, R, O, st) == INVALID      # NULL wavelengths with k > 1
    assert f(cam._h, 64, 0, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 9, S, W, None, 0, R, O, st) == INVALID
    assert f(None, 64, 1, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, None, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, S + 4, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, S, W + 2, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, S, W, S + 8, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, S, W, None, 0, None, O, st) == INVALID
    assert f(cam._h, 64, 1, S, W, None, 0, R + 4, O, st) == INVALID
    assert f(cam._h, 64, 1, S, W, None, 0, R, None, st) == INVALID
    assert f(cam._h, 64, 1, S, W, None, 0, R, O + 2, st) == INVALID
    torch.cuda.synchronize()
    r64, w64 = r[:64].contiguous(), w[:64].contiguous()
    with pytest.raises(ValueError):
        cam.transmittance(s, r64, wavelengths=w64.double())
    with pytest.raises(ValueError):
        cam.transmittance(s, r64, wavelengths=w[:65].contiguous())      # 65 for 64 samples
    with pytest.raises(ValueError):
        cam.transmittance(s, r64, wavelengths=w64.view(32, 2))
    with pytest.raises(ValueError):
        cam.transmittance(s, r64, wavelengths=w[:128].view(64, 2))      # (n, 2) wavelengths need (n, 2, 8) records
    with pytest.raises(TypeError):
        cam.transmittance(s, r64, wavelengths=np.full(64, 500.0, F32))
    with pytest.raises(ZoicError):
        cam.transmittance(s, torch.zeros((64, 9, 8), device="cuda"), wavelengths=torch.full((64, 9), 500.0, device="cuda"))
    assert tuple(cam.transmittance(s, r64).shape) == (64,)
    assert tuple(cam.transmittance(s, r[:128].view(64, 2, 8), wavelengths=w[:128].view(64, 2)).shape) == (64, 2)
    cam.close()

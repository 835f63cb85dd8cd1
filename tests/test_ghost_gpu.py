"""Ghost rays on the MI355X (zoic_create_ghost_rays_device): the kernel gives the host build of csrc/ghost.hpp bit for bit on all
n x p x 8 words -- the starts from the CPU reference of the hero call at k = 1 (tests/hero_ref.py) or from differentials_ref.kolb_start
-- with and without coatings, on STRICT and FAST cameras, in the d-line form and at a wavelength per sample; the columns without a
start, without a wavelength or without a valid pair get the documented dead record; the other lens models, split calls and the error
codes are the header's; the records and the counters are left alone.

Sizes: 1, 63, 65 and 4096 samples at p = 1, 3 and all 21 pairs of C2 and at p = 8 on C3, and 524 353 = 2048 x 256 + 65 samples at
p = 1, the first size at which the grid-stride loop takes a second turn and that turn ends in a partial wave."""
import ctypes as C

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera, _capi
from zoic_amd.workloads import ray_rng_states

import differentials_ref as dref
import ghost_ref as gref
import hero_cases as hr
import host_drivers
from device_cases import BIG, bits_f32 as _bits, camera as _camera, oracle as _oracle, params as _params, samples as _samples
from hero_cases import LOSS_CAMERAS as CAMERAS, loss_reference as _reference
from host_drivers import run_ghost_records as run_records
from spectral_ref import BAD, LAMBDA_D32, WAVES
from transmittance_ref import films_where_media_differ

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 4096
SIZES = [1, 63, 65, N]


@pytest.fixture(scope="module")
def driver():
    return host_drivers.ghost()


_TABLES = {}


def _tables(name):
    """(lens geometry, dispersion, film in trace order, the pairs that reflect (m, 2)) of the camera's lens, from a tables-only camera"""
    if name not in _TABLES:
        cam = hr.spec(name).camera(device=-1)
        info, disp, pairs = cam.info(), cam.dispersion(), cam.ghost_pairs()
        cam.close()
        _TABLES[name] = gref.lens(info), disp, films_where_media_differ(disp), pairs
    return _TABLES[name]


def _coat(cam, name, coated):
    if coated:
        nc, l0 = _tables(name)[2]
        cam.set_coatings(nc[::-1], l0[::-1])      # file order
    return cam


def _expected(driver, name, coated, starts, lam, weights, pairs):
    """(n, p, 8) float32: the host build's records of the call's columns"""
    L, disp, film, _ = _tables(name)
    return run_records(driver, L, disp, lam, starts[:, 0:3], starts[:, 3:6], pairs, have=weights != 0, film=film if coated else None)


def _dead(reason, interface=0, leg=0):
    rec = np.zeros(8, np.uint32)
    rec[7] = gref.flag_word(reason, interface, leg)
    return rec


# ---- host == device bits, n x p x 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [PRECISION_STRICT, PRECISION_FAST], ids=["strict", "fast"])
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_kernel_equals_the_host_build(gpu, oracle_lib, driver, cfg, coated, precision):
    """every word of n = 1, 63, 65 and 4096 samples at a wavelength per sample: p = 1, 3 and all 21 pairs on C2, p = 8 on C3.  STRICT
    records are the reference's, so every row is compared; a FAST record may end at another try than the reference's (then its start
    is not the recorded one): those rows, fewer than 1 in 1000, are left to the STRICT case"""
    import torch
    name = CAMERAS[cfg]
    s, lam, st, words, starts = _reference(oracle_lib, name, 1)
    every = _tables(name)[3]
    columns = [every[10:11], every[[2, 20, 7]], every] if cfg == "C2" else [every[[0, 44, 9, 17, 23, 30, 38, 5]]]
    assert cfg != "C2" or len(every) == 21
    cam = _coat(hr.spec(name).camera(precision=precision), name, coated)
    traced = dead = 0
    for n in SIZES:
        ts, tl = torch.from_numpy(np.array(s[:n])).cuda(), torch.from_numpy(np.array(lam[:n])).cuda()
        tst = torch.from_numpy(np.array(st[:n]).view(np.int32)).cuda()
        rays = cam.create_rays_hero(ts, tl, rng_states=tst)["rays"].view(n, 8)
        r = rays.cpu().numpy()
        known = r[:, 7].view(np.uint32) == words[:n, 0, 7]               # the flag word: the try count among it
        if precision == PRECISION_STRICT:
            assert hr.same_words(r.view(np.uint32).reshape(n, 1, 8), words[:n]).all()
        else:
            assert known.mean() >= 0.999 or n < 1000
        for pairs in columns:
            got = cam.create_ghost_rays(ts, rays, pairs, wavelengths=tl.view(n), rng_states=tst)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (n, len(pairs), 8) and got.dtype == torch.float32
            g = got.cpu().numpy()
            want = _expected(driver, name, coated, starts[:n], lam[:n, 0], r[:, 6], pairs)
            assert np.array_equal(_bits(g[known]), _bits(want[known])), (n, len(pairs), np.argwhere(_bits(g) != _bits(want))[:8].tolist())
            flags = _bits(g[known][..., 7])
            traced += int((flags == 1).sum())
            dead += int((flags != 1).sum())
    assert traced >= 1000 and dead >= 1000
    cam.close()


@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
def test_d_line_form(gpu, oracle_lib, driver, coated):
    """wavelengths=None on create_rays records, the library's own retry streams at a ray_index_base: the host build from kolb_start at
    587.5618 nm, bit for bit, all 21 pairs; and the same bits from the call given that wavelength per sample"""
    import torch
    p = _params("C2")
    cam = _coat(_camera(p), "C2", coated)
    pairs = _tables("C2")[3]
    oc = _oracle(oracle_lib, p)
    for n in SIZES:
        base = 5
        s = _samples(n, seed=11)
        states = ray_rng_states(n, seed=1, ray_index_base=base)      # the streams the library derives itself (seed 1)
        ts = torch.from_numpy(s).cuda()
        rays = cam.create_rays(ts, ray_index_base=base)["rays"]
        got = cam.create_ghost_rays(ts, rays, pairs, ray_index_base=base)
        lam = torch.full((n,), float(LAMBDA_D32), device="cuda")
        same = cam.create_ghost_rays(ts, rays, pairs, wavelengths=lam, ray_index_base=base)
        assert torch.equal(got.view(torch.int32), same.view(torch.int32))
        r, g = rays.cpu().numpy(), got.cpu().numpy()
        live = np.nonzero(r[:, 6] != 0)[0]
        tries = ((r[live, 7].view(np.uint32) >> 1) & 31).astype(np.int64)
        starts = np.zeros((n, 6), F32)
        if len(live):
            o0, d0 = dref.kolb_start(oc, p, s[live], tries, states[live], oracle_lib)
            starts[live, 0:3], starts[live, 3:6] = o0, d0
        want = _expected(driver, "C2", coated, starts, np.full(n, LAMBDA_D32), r[:, 6], pairs)
        assert np.array_equal(_bits(g), _bits(want)), (n, np.argwhere(_bits(g) != _bits(want))[:8].tolist())
    cam.close()


def test_second_grid_turn_and_ragged_wave(gpu, oracle_lib, driver):
    """n = 2048 x 256 + 65, p = 1, the library's own retry streams: all rows against the two-pass identity (the same bits from calls on
    the two halves, the second starting in the middle of a wave), 16 Ki random rows and the last 129 against the host build from
    kolb_start"""
    import torch
    p = _params("C2")
    cam = _coat(_camera(p), "C2", True)
    base = 1000
    pair = _tables("C2")[3][13:14]                 # (6, 3): leg 1 crosses the stop; about four in ten of its ghosts come through
    assert tuple(pair[0]) == (6, 3)
    s = _samples(BIG, seed=7)
    lam = np.resize(WAVES, BIG).astype(F32)
    states = ray_rng_states(BIG, seed=1)           # seed 1, no base: the streams the library derives itself ...
    ts, tl = torch.from_numpy(s).cuda(), torch.from_numpy(lam).cuda()
    rays = cam.create_rays(ts, wavelengths=tl)["rays"]
    got = cam.create_ghost_rays(ts, rays, pair, wavelengths=tl)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (BIG, 1, 8)
    g, r = got.cpu().numpy(), rays.cpu().numpy()
    idx = np.unique(np.r_[np.random.RandomState(1).choice(BIG, 1 << 14, replace=False), BIG - 129:BIG])
    live = idx[r[idx, 6] != 0]
    tries = ((r[live, 7].view(np.uint32) >> 1) & 31).astype(np.int64)
    assert int((tries > 0).sum()) >= 200
    oc = _oracle(oracle_lib, p)
    o0, d0 = dref.kolb_start(oc, p, s[live], tries, states[live], oracle_lib)
    want = _expected(driver, "C2", True, np.concatenate([o0, d0], 1), lam[live], r[live, 6], pair)
    assert np.array_equal(_bits(g[live]), _bits(want))
    assert (_bits(want[..., 7]) == 1).sum() >= 1000
    none = r[:, 6] == 0
    assert none.any() and (_bits(g[none, 0]) == _dead(gref.NO_START)).all()
    assert (r[BIG - 65:, 6] != 0).any()
    # ... and two halves at their ray_index_base, the second starting in the middle of a wave
    rays_b = cam.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    whole = cam.create_ghost_rays(ts, rays_b, pair, wavelengths=tl, ray_index_base=base)
    cut = BIG // 2 + 7
    parts = [cam.create_ghost_rays(ts[lo:hi].contiguous(), rays_b[lo:hi].contiguous(), pair, wavelengths=tl[lo:hi].contiguous(), ray_index_base=base + lo)
             for lo, hi in ((0, cut), (cut, BIG))]
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32))
    cam.close()


# ---- dead columns ---------------------------------------------------------------------------------------------------------------
def test_dead_columns(gpu, oracle_lib, driver):
    """main records of weight 0, wavelengths outside [360, 830] and NaN, invalid pairs and pairs on the stop, each mixed into live waves
    and filling waves with no live lane: the exact dead record, +0.0 and the documented flag word; every word against the host build"""
    import torch
    name = "C2"
    L, disp, film, every = _tables(name)
    stop, count = L["stop"], L["count"]
    a, b = (int(v) for v in every[13])                                       # (6, 3) around the stop at 4
    assert b < stop < a
    pairs = np.array([(a, b), (a, a), (b, a), (count, 0), (200, 100), (a, stop), (stop, b), every[3]], np.int64)
    s, lam, st, words, starts = _reference(oracle_lib, name, 1)
    cam = _coat(hr.spec(name).camera(), name, True)
    ts, tl = torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(lam)).cuda()
    tst = torch.from_numpy(np.array(st).view(np.int32)).cuda()
    rays = cam.create_rays_hero(ts, tl, rng_states=tst)["rays"].view(N, 8).clone()
    w0 = rays[:, 6].cpu().numpy()
    assert (w0 == 0).sum() >= 100                                            # records of weight 0 of the forward call's own ...
    rays[64:128, 6] = 0.0                                                    # ... and a whole wave of them
    here = np.array(lam[:, 0])
    live_rows = np.nonzero(w0 != 0)[0]
    mixed = live_rows[(live_rows >= 320) & (live_rows < 384)][:len(BAD)]
    assert len(mixed) == len(BAD)
    here[mixed] = BAD                                                        # single lanes of a live wave
    here[448:512] = np.resize(BAD, 64)                                       # a whole wave
    assert (w0[448:512] != 0).any()
    got = cam.create_ghost_rays(ts, rays, pairs, wavelengths=torch.from_numpy(here).cuda(), rng_states=tst).cpu().numpy()
    r = rays.cpu().numpy()
    want = _expected(driver, name, True, starts, here, r[:, 6], pairs)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8].tolist()
    g = _bits(got)
    for j in (1, 2, 3, 4):
        assert (g[:, j] == _dead(gref.INVALID_PAIR)).all()                   # whatever the row holds
    none = r[:, 6] == 0
    for j in (0, 5, 6, 7):
        assert (g[none, j] == _dead(gref.NO_START)).all() and none[64:128].all()
        assert (g[448:512, j][~none[448:512]] == _dead(gref.WAVELENGTH)).all() and (g[mixed, j] == _dead(gref.WAVELENGTH)).all()
    ok = ~none & hr.valid(here)
    assert (g[ok, 5] == _dead(gref.NO_REFLECTION, stop, 1)).all() and (g[ok, 6] == _dead(gref.NO_REFLECTION, stop, 0)).all()
    assert ((g[ok, 0, 7] & 1) == 1).sum() >= 100 and ((g[ok, 7, 7] & 1) == 1).sum() >= 100
    cam.close()


# ---- the other lens models ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [dict(lensModel=0), dict(lensModel=0, useDof=False), dict(lensModel=2)], ids=["thin", "thin-noDOF", "none"])
def test_other_lens_models_give_reason_model(gpu, over):
    import torch
    cam = _camera(_params("C2"))
    n = 4096 + 65
    s = torch.from_numpy(_samples(n, seed=19)).cuda()
    rays = cam.create_rays(s)["rays"]
    cam.update(**_params("C2", **over))
    if over["lensModel"] == 0:
        rays = cam.create_rays(s)["rays"]
    pairs = np.array([(3, 1), (1, 3), (7, 0)])
    lam = torch.full((n,), 500.0, device="cuda")
    for w in (None, lam):
        got = cam.create_ghost_rays(s, rays, pairs, wavelengths=w).cpu().numpy()
        assert (_bits(got) == _dead(gref.MODEL)).all()
    assert cam.ghost_pairs().shape == (0, 2)
    cam.close()


# ---- records and counters untouched, more than 32 pairs -------------------------------------------------------------------------
def test_records_untouched_and_forty_pairs(gpu):
    """on the camera without the exit-pupil LUT (half of its records retry: the streams matter): the records, the inputs and the
    camera's counters are bitwise what they were; 40 pairs through Python equal a 32-pair call beside an 8-pair call; the film table
    is read at the call"""
    import torch
    name = "C2-nolut"
    cam = hr.spec(name).camera()
    n, base = N + 37, 777
    s = hr.samples(n, 5)
    lam = WAVES[np.arange(n) % len(WAVES)].astype(F32)
    ts, tl = torch.from_numpy(s).cuda(), torch.from_numpy(lam).cuda()
    rays = cam.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    before = cam.counters()
    keep = [t.clone() for t in (ts, tl, rays)]
    every = cam.ghost_pairs()
    forty = np.concatenate([every, every[::-1][:19]])
    assert len(every) == 21 and len(forty) == 40
    all40 = cam.create_ghost_rays(ts, rays, forty, wavelengths=tl, ray_index_base=base)
    a32 = cam.create_ghost_rays(ts, rays, forty[:32], wavelengths=tl, ray_index_base=base)
    a8 = cam.create_ghost_rays(ts, rays, forty[32:], wavelengths=tl, ray_index_base=base)
    assert tuple(all40.shape) == (n, 40, 8)
    assert torch.equal(all40.view(torch.int32), torch.cat([a32, a8], 1).view(torch.int32))
    traced = (all40[:, :21, 7].view(torch.int32) & 1) == 1
    assert int(traced.sum()) >= 1000
    wrong = cam.create_ghost_rays(ts, rays, every, wavelengths=tl, ray_index_base=base + 1)       # another stream: other starts for the retried
    assert not torch.equal(wrong.view(torch.int32), all40[:, :21].contiguous().view(torch.int32))
    count = cam.info()["lensCount"]
    cam.set_coatings(np.full(count, 1.38, F32), 550.0)
    film = cam.create_ghost_rays(ts, rays, every, wavelengths=tl, ray_index_base=base)
    assert torch.equal((film[:, :, 7].view(torch.int32) & 1) == 1, traced)                       # a film changes no path ...
    assert float(film[:, :, 6][traced].mean()) < float(all40[:, :21, 6][traced].mean())          # ... and weakens the ghosts
    cam.set_coatings(None, None)
    again = cam.create_ghost_rays(ts, rays, every, wavelengths=tl, ray_index_base=base)
    assert torch.equal(again.view(torch.int32), all40[:, :21].contiguous().view(torch.int32))
    torch.cuda.synchronize()
    for x, y in zip(keep, (ts, tl, rays)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert cam.counters() == before
    assert ((rays[:, 7].view(torch.int32) >> 1) & 31).gt(0).sum() >= 1000
    cam.close()


def test_error_codes(gpu):
    import torch
    lib = gpu
    OK, INVALID, NOT_UPDATED = 0, _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT"), _capi.STATUS_NAMES.index("ZOIC_ERR_NOT_UPDATED")
    cam = ZoicCamera(device=0)
    s = torch.zeros((64, 4), device="cuda")
    r = torch.zeros((64 + 1, 8), device="cuda")
    o = torch.zeros((64 * 32 + 1, 8), device="cuda")
    w = torch.full((64 + 1,), 500.0, device="cuda")
    pairs = np.array([3 | 1 << 8] * 33, np.uint32)
    st = C.c_void_p(0)
    f = lib.zoic_create_ghost_rays_device
    S, R, O, W, P = s.data_ptr(), r.data_ptr(), o.data_ptr(), w.data_ptr(), pairs.ctypes.data
    assert f(cam._h, 64, 1, P, S, W, None, 0, R, O, st) == NOT_UPDATED
    assert f(cam._h, 64, 0, P, S, W, None, 0, R, O, st) == INVALID        # p first
    cam.update(**_params("C2"))
    assert f(cam._h, 0, 1, None, None, None, None, 0, None, None, st) == OK
    assert f(cam._h, 0, 33, None, None, None, None, 0, None, None, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, None, 0, R, O, st) == OK
    assert f(cam._h, 64, 1, P, S, None, None, 0, R, O, st) == OK           # the d-line form
    assert f(cam._h, 64, 32, P, S, W, None, 0, R, O, st) == OK
    assert f(cam._h, 64, 2, P + 4, S, W + 4, None, 0, R + 32, O + 32, st) == OK
    assert f(cam._h, 64, 0, P, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 33, P, S, W, None, 0, R, O, st) == INVALID
    assert f(None, 64, 1, P, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, None, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P + 2, S, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P, None, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S + 4, W, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W + 2, None, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, S + 8, 0, R, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, None, 0, None, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, None, 0, R + 4, O, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, None, 0, R, None, st) == INVALID
    assert f(cam._h, 64, 1, P, S, W, None, 0, R, O + 8, st) == INVALID
    torch.cuda.synchronize()
    r64, w64 = r[:64].contiguous(), w[:64].contiguous()
    one = np.array([(3, 1)])
    with pytest.raises(ValueError):
        cam.create_ghost_rays(s, r64, one, wavelengths=w64.double())
    with pytest.raises(ValueError):
        cam.create_ghost_rays(s, r64, one, wavelengths=w[:65].contiguous())
    with pytest.raises(ValueError):
        cam.create_ghost_rays(s, r[:65].contiguous(), one)
    with pytest.raises(TypeError):
        cam.create_ghost_rays(s, r64, one, wavelengths=np.full(64, 500.0, F32))
    for bad in (np.zeros((0, 2), np.int64), np.array([3, 1]), np.array([(3.0, 1.0)]), np.array([(-1, -1)]), np.array([(256, 0)])):
        with pytest.raises(ValueError):
            cam.create_ghost_rays(s, r64, bad)
    assert tuple(cam.create_ghost_rays(s, r64, one).shape) == (64, 1, 8)
    cam.close()

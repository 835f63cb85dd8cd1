"""Hero-wavelength rays on the MI355X (zoic_create_rays_hero_device): column 0 is the spectral call bit for bit, counters included; a
companion is the hero's accepted start traced once at its own wavelength -- the record of the CPU reference of the whole call
(tests/hero_ref.py) on every row, which is the CPU oracle's own record where the oracle accepts the same try at that wavelength and a
lost record where it needs a later one; a companion at the hero's wavelength repeats the hero's record; FAST
agrees with STRICT; live companions trace back to the hero's screen sample; rejected wavelengths, the thin lens, determinism, launch
splits and the error codes behave as the header states.

The reference of every bit-exact claim about a companion is the oracle through fuzz_cameras._oracle_spectral (STRICT, one wavelength
at a time), never the kernel under test."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, RAY_COMPANION_LOST, ZoicCamera, _capi
from zoic_amd.workloads import ray_rng_states

import backward_spectral_ref as bs
from fuzz_cameras import _oracle_spectral, same_bits
from hero_ref import hero_reference, same_words, words_of as _words
from device_cases import bits_f32 as _bits, camera as _camera, delta as _delta, params as _params, samples as _samples
from spectral_ref import BAD, LAMBDA_D, WAVES

pytestmark = pytest.mark.gpu

N = 1 << 14
LOST = RAY_COMPANION_LOST
COLUMNS = np.array([550.0, 450.0, 650.0, 400.0], np.float32)   # hero first


def _abbe(p, v):
    return np.full(ZoicCamera(device=-1).update(**dict(p, useImage=False)).info()["lensCount"], v, np.float32)


def _cam(cfg, precision=PRECISION_STRICT, **over):
    """cfg "C3" gets V = 50 everywhere (DOUBLE_GAUSS ships no V-numbers); C1's thin lens gets a vignetting distance: its rejection loop runs"""
    if cfg == "C1":
        over = dict(dict(opticalVignettingDistance=5.0), **over)
    p = _params(cfg, **over)
    return _camera(p, precision, _abbe(p, 50.0) if cfg == "C3" else None), p


def _hero_waves(n, k, seed=1):
    """hero wavelengths cycle WAVES, companions anywhere in the valid range"""
    w = np.random.RandomState(seed).uniform(360.0, 830.0, (n, k)).astype(np.float32)
    w[:, 0] = np.resize(WAVES, n)
    return w


def _column_equals(hero, j, ref):
    assert np.array_equal(hero["flags"][:, j], ref["flags"])
    assert np.array_equal(_bits(hero["planes"][:, :, j]), _bits(ref["planes"]))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C5"])
def test_hero_column_is_the_spectral_call(cfg):
    """STRICT and FAST: both calls run one kernel body, so column 0 and the counters are the spectral call's in every bit in FAST too"""
    s_all, st_all = _samples(N, seed=11), ray_rng_states(N, seed=2)
    for precision in (PRECISION_STRICT, PRECISION_FAST):
        cam, _ = _cam(cfg, precision)
        for n in (N, 1, 63, 64, 65, 257):   # a partial wave, the chunk edge at 256, a lane that holds several rays in turn
            s, st = s_all[:n], st_all[:n]
            w = _hero_waves(n, 4)
            ref, cr = _delta(cam, lambda: cam.create_rays(s, rng_states=st, wavelengths=w[:, 0].copy(), ray_index_base=3))
            got, cg = _delta(cam, lambda: cam.create_rays_hero(s, w, rng_states=st, ray_index_base=3))
            assert got["rays"].shape == (n, 4) and got["planes"].shape == (7, n, 4)
            _column_equals(got, 0, ref)
            assert cg == cr, (precision, n, cg, cr)
            one, c1 = _delta(cam, lambda: cam.create_rays_hero(s, w[:, :1].copy(), rng_states=st, ray_index_base=3))
            assert one["rays"].shape == (n, 1)
            _column_equals(one, 0, ref)
            assert c1 == cr
        cam.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,over", [("C2", {}), ("C5", {}), ("C2", dict(useImage=True)), ("C3", {})], ids=["C2", "C5", "tessar-bokeh", "C3-V50"])
def test_companions_against_the_oracle(oracle_lib, cfg, over):
    cam, p = _cam(cfg, **over)
    disp = cam.dispersion()
    assert disp["cauchy_b"].any()
    s, st = _samples(N, seed=11), ray_rng_states(N, seed=2)
    w = np.tile(COLUMNS, (N, 1))
    got = cam.create_rays_hero(s, w, rng_states=st)
    cam.close()
    ref = [_oracle_spectral(oracle_lib, p, disp, s, np.ascontiguousarray(w[:, j]), st)[0] for j in range(4)]
    # every record of every row, those the try counts say nothing about included: the CPU reference of the whole call
    want, _ = hero_reference(oracle_lib, p, disp, s, w, st)
    assert same_words(_words(got), want).all(), int((~same_words(_words(got), want)).sum())
    tries = [((r["flags"] >> 1) & 31).astype(np.int32) for r in ref]
    # the hero is the oracle's ray at the hero's wavelength
    assert np.array_equal(got["flags"][:, 0], ref[0]["flags"])
    assert same_bits(got["planes"][:, :, 0], ref[0]["planes"]).all()
    hflags = got["flags"][:, 0]
    live = got["weight"][:, 0] != 0
    assert live.sum() > N // 8
    lost_total = retried_checked = 0
    for j in (1, 2, 3):
        f, pl = got["flags"][:, j], got["planes"][:, :, j]
        same = live & (tries[j] == tries[0])
        later = live & (tries[j] > tries[0])
        earlier = live & (tries[j] < tries[0])
        print("%s column %d (%g nm): live %d, same try %d (retried %d), lost %d, left out %d" %
              (cfg, j, COLUMNS[j], live.sum(), same.sum(), (same & (tries[0] > 0)).sum(), later.sum(), earlier.sum()))
        assert earlier.sum() <= 0.02 * live.sum(), (j, earlier.sum(), live.sum())   # about the inputs: the try counts decide nearly every row
        assert same_bits(pl[:, same], ref[j]["planes"][:, same]).all(), (j, int((~same_bits(pl[:, same], ref[j]["planes"][:, same]).all(0)).sum()))
        assert np.array_equal(f[same], hflags[same])
        assert (_bits(pl[:, later]) == 0).all() and np.array_equal(f[later], hflags[later] | LOST)
        # heroes of weight 0: no start to share
        assert (_bits(pl[:, ~live]) == 0).all() and np.array_equal(f[~live], hflags[~live] | LOST)
        lost_total += int(later.sum())
        retried_checked += int((same & (tries[0] > 0)).sum())
    assert lost_total >= 1
    if not over:
        assert retried_checked >= 500, retried_checked


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [PRECISION_STRICT, PRECISION_FAST], ids=["strict", "fast"])
@pytest.mark.parametrize("cfg", ["C5", "C3"])
def test_same_wavelength_same_record(cfg, precision):
    cam, _ = _cam(cfg, precision)
    s, st = _samples(N, seed=11), ray_rng_states(N, seed=2)
    w = _hero_waves(N, 3, seed=3)
    w[:, 0] = np.random.RandomState(4).uniform(400.0, 700.0, N).astype(np.float32)
    w[:, 1] = w[:, 0]
    w[:, 2] = LAMBDA_D
    got = cam.create_rays_hero(s, w, rng_states=st)
    cam.close()
    words = _words(got)
    live = got["weight"][:, 0] != 0
    # every hero that has a start to share, retried ones included; a hero of weight 0 has none and the header gives its companions
    # lost records whatever their wavelength (test_companions_against_the_oracle holds the same rows to that)
    assert np.array_equal(words[live, 1], words[live, 0])
    assert (words[~live, 1, :7] == 0).all() and np.array_equal(words[~live, 1, 7], words[~live, 0, 7] | LOST)
    assert (live & (got["tries"][:, 0] > 0)).sum() > 100          # retried heroes are among them
    assert not np.array_equal(words[live, 2], words[live, 0])    # and another wavelength is another ray


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C2", "C5", "C3"])
def test_fast_agrees_with_strict_on_companions(cfg):
    n, k = 1 << 18, 4
    strict, _ = _cam(cfg, PRECISION_STRICT)
    fast, _ = _cam(cfg, PRECISION_FAST)
    assert not fast.info()["fastRunsStrict"]
    s = _samples(n, seed=21)
    w = np.random.RandomState(4).uniform(400.0, 700.0, (n, k)).astype(np.float32)
    a = strict.create_rays_hero(s, w)
    b = fast.create_rays_hero(s, w)
    strict.close(); fast.close()
    differ = (a["flags"] != b["flags"]) | (a["weight"] != b["weight"])
    print("%s: %d of %d records differ in flags or weight" % (cfg, differ.sum(), differ.size))
    assert differ.mean() <= 5e-5, differ.sum()
    live = ~differ & (a["weight"] != 0) & np.isfinite(a["dir"]).all(0)
    assert live[:, 1:].sum() > n // 8
    err = (a["dir"][:, live].astype(np.float64) - b["dir"][:, live]) ** 2
    rmse = np.sqrt(err.sum(0).mean())
    print("%s: direction RMSE %.3g over %d live records" % (cfg, rmse, live.sum()))
    assert rmse < 1e-5
    assert not np.array_equal(_bits(a["planes"][:, live]), _bits(b["planes"][:, live]))   # FAST is not the STRICT kernel


def test_fast_runs_strict_camera_gives_strict_bits():
    strict, _ = _cam("C2", PRECISION_STRICT, focalLength=-10.0)   # negative focal-length ratio: outside the FAST modes' domain
    fast, _ = _cam("C2", PRECISION_FAST, focalLength=-10.0)
    assert fast.info()["fastRunsStrict"]
    s = _samples(N, seed=8)
    w = np.random.RandomState(5).uniform(400.0, 700.0, (N, 4)).astype(np.float32)
    a, b = strict.create_rays_hero(s, w), fast.create_rays_hero(s, w)
    strict.close(); fast.close()
    assert np.array_equal(_words(a), _words(b))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_of_the_companions():
    """C5, FAST, device tensors: every live companion outside the edge set traces back, at its own wavelength, to the hero's (sx, sy)
    within the bound tests/test_backward_spectral_gpu.py::test_round_trip_with_the_forward_spectral_kernel derives: 2 x the d-line
    round trip's maximum, measured here on the same samples with the existing calls; the edge set is TraceBack.edge's."""
    import torch
    cam, p = _cam("C5", PRECISION_FAST)
    host = ZoicCamera(device=-1).update(**p)
    T = bs.SpectralTraceBack(host.info(), p, host.dispersion())
    host.close()
    s = _samples(N, seed=11)
    smp = torch.from_numpy(s).to("cuda:0")
    st = torch.from_numpy(ray_rng_states(N, seed=2).view(np.int32)).to("cuda:0")
    fwd0 = cam.create_rays(smp, rng_states=st)
    scr0, fl0 = cam.trace_back(fwd0)
    torch.cuda.synchronize()
    rec0 = fwd0["rays"].cpu().numpy()
    live0 = rec0[:, 6] > 0
    keep0 = ~T.edge(T.trace(rec0[live0, 0:3], rec0[live0, 3:6])) & ((fl0.cpu().numpy()[live0] & 1) == 1)
    d_max = float(np.abs(scr0.cpu().numpy()[live0].astype(np.float64) - s[live0, :2]).max(1)[keep0].max())
    k = len(COLUMNS)
    lam_h = np.tile(COLUMNS, (N, 1))
    lam = torch.from_numpy(lam_h).to("cuda:0")
    res = cam.create_rays_hero(smp, lam, rng_states=st)
    assert tuple(res["rays"].shape) == (N, k, 8) and tuple(res["flags"].shape) == (N, k) and tuple(res["origin"].shape) == (3, N, k)
    scr, fl = cam.trace_back(res["rays"].view(N * k, 8), wavelengths=lam.view(N * k))
    torch.cuda.synchronize()
    rec = res["rays"].cpu().numpy()
    scr, fl = scr.cpu().numpy().reshape(N, k, 2), fl.cpu().numpy().astype(np.uint32).reshape(N, k)
    cam.close()
    comp = np.zeros((N, k), bool)
    comp[:, 1:] = rec[:, 1:, 6] > 0
    assert comp.sum() >= 4096
    ref = T.trace_at(rec[comp][:, 0:3], rec[comp][:, 3:6], lam_h[comp])
    edge = T.edge(ref)
    assert edge.mean() <= 0.02, edge.mean()
    ok = (fl[comp] & 1) == 1
    assert ok[~edge].all(), int((~ok & ~edge).sum())
    target = np.broadcast_to(s[:, None, :2], (N, k, 2))[comp].astype(np.float64)
    rt = np.abs(scr[comp].astype(np.float64) - target).max(1)[~edge]
    print("companion round trip: %d rays, max %.3g = %.2f x the d-line round trip's max (%.3g); edge share %.2f %%" %
          (len(rt), rt.max(), rt.max() / d_max, d_max, 100 * edge.mean()))
    assert rt.max() <= 2.0 * d_max, (rt.max(), d_max)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_rejections_and_counters(cfg):
    n, k = 4096, 4
    cam, _ = _cam(cfg)
    s, st = _samples(n, seed=13), ray_rng_states(n, seed=2)
    good = np.random.RandomState(6).uniform(360.0, 830.0, (n, k)).astype(np.float32)
    rows = np.arange(len(BAD)) * 97 + 5
    cols = 1 + np.arange(len(BAD)) % (k - 1)
    ref, cref = _delta(cam, lambda: cam.create_rays_hero(s, good, rng_states=st))
    assert not (ref["flags"] == 0x80).any()
    # a bad companion: that column only
    w = good.copy()
    w[rows, cols] = BAD
    got, cgot = _delta(cam, lambda: cam.create_rays_hero(s, w, rng_states=st))
    hit = np.zeros((n, k), bool)
    hit[rows, cols] = True
    a, b = _words(got), _words(ref)
    assert (a[hit][:, :7] == 0).all() and (a[hit][:, 7] == 0x80).all()
    assert np.array_equal(a[~hit], b[~hit])
    assert cgot == cref
    # a bad hero: the whole row, and the counters of the spectral call on column 0
    w = good.copy()
    w[rows, 0] = BAD
    got, cgot = _delta(cam, lambda: cam.create_rays_hero(s, w, rng_states=st))
    _, cspec = _delta(cam, lambda: cam.create_rays(s, rng_states=st, wavelengths=w[:, 0].copy()))
    a = _words(got)
    assert (a[rows][:, :, :7] == 0).all() and (a[rows][:, :, 7] == 0x80).all()
    keep = np.ones(n, bool)
    keep[rows] = False
    assert np.array_equal(a[keep], b[keep])
    assert cgot == cspec
    # the counters never depend on the companions' wavelengths
    other = good.copy()
    other[:, 1:] = np.random.RandomState(7).uniform(360.0, 830.0, (n, k - 1)).astype(np.float32)
    other[::5, 2] = np.nan
    _, cother = _delta(cam, lambda: cam.create_rays_hero(s, other, rng_states=st))
    assert cother == cref
    cam.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_thin_lens_ignores_the_wavelengths():
    cam, _ = _cam("C1")
    s = _samples(N, seed=19)
    plain, cp = _delta(cam, lambda: cam.create_rays(s, ray_index_base=11))
    w = np.random.RandomState(8).uniform(360.0, 830.0, (N, 5)).astype(np.float32)
    got, cg = _delta(cam, lambda: cam.create_rays_hero(s, w, ray_index_base=11))
    cam.close()
    assert (plain["weight"] == 0).any() and (plain["weight"] != 0).any()
    for j in range(5):
        _column_equals(got, j, plain)
    assert cg == cp


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_split_launches():
    import torch
    n, k = N + 200, 4                     # n / 2 = 8292 is no multiple of the 256-sample chunk
    half = n // 2
    assert half % 256 != 0
    cam, _ = _cam("C5", PRECISION_FAST)
    s = torch.from_numpy(_samples(n, seed=17)).cuda()
    lam = torch.from_numpy(np.random.RandomState(7).uniform(400.0, 700.0, (n, k)).astype(np.float32)).cuda()
    whole = cam.create_rays_hero(s, lam, ray_index_base=1000)["rays"].clone()      # rng_states=None: the keyed streams
    again = cam.create_rays_hero(s, lam, ray_index_base=1000)["rays"].clone()
    parts = torch.empty_like(whole)
    for a, b in ((0, half), (half, n)):
        parts[a:b] = cam.create_rays_hero(s[a:b].contiguous(), lam[a:b].contiguous(), ray_index_base=1000 + a)["rays"]
    # ray i draws from the stream keyed by ray_index_base + i, not i k: column 0 is the spectral call with the same base
    spec = cam.create_rays(s, wavelengths=lam[:, 0].contiguous(), ray_index_base=1000)["rays"].clone()
    torch.cuda.synchronize()
    cam.close()
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    assert torch.equal(whole[:, 0].contiguous().view(torch.int32), spec.view(torch.int32))
    assert (whole[:, 0, 7].view(torch.int32) & 1).sum().item() > 100               # retried heroes: the streams were drawn from


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    L = _capi.load()
    INVALID, NOT_UPDATED = (_capi.STATUS_NAMES.index(x) for x in ("ZOIC_ERR_INVALID_ARGUMENT", "ZOIC_ERR_NOT_UPDATED"))
    cam = ZoicCamera(device=0)
    n, k = 64, 4
    s = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    lam = torch.full((n * k + 1,), LAMBDA_D, dtype=torch.float32, device="cuda")
    st = torch.ones((n + 1, 4), dtype=torch.int32, device="cuda")
    out = torch.empty((n * k + 1, 8), dtype=torch.float32, device="cuda")

    def call(n=n, k=k, s=s.data_ptr(), w=lam.data_ptr(), r=None, o=out.data_ptr()):
        return L.zoic_create_rays_hero_device(cam._h, n, k, s, w, r, 0, o, None)
    assert call() == NOT_UPDATED
    assert call(k=0) == INVALID                     # k is checked first
    cam.update(**_params("C2"))
    for kw in (dict(k=0), dict(k=9), dict(s=None), dict(w=None), dict(o=None), dict(s=s.data_ptr() + 4), dict(w=lam.data_ptr() + 2),
               dict(r=st.data_ptr() + 4), dict(o=out.data_ptr() + 8), dict(k=1, w=None), dict(k=1, o=out.data_ptr() + 8)):
        assert call(**kw) == INVALID, kw
    assert call(n=0) == 0 and call(n=0, k=1) == 0
    assert call(k=0, n=0) == INVALID
    assert call() == 0
    assert call(w=lam.data_ptr() + 4, r=st.data_ptr() + 16, s=s.data_ptr() + 16, o=out.data_ptr() + 32) == 0
    assert call(k=8, n=n * k // 8) == 0
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        cam.create_rays_hero(s[:n].contiguous(), np.full((n, k), LAMBDA_D, np.float32))
    with pytest.raises(ValueError):
        cam.create_rays_hero(s[:n].contiguous(), lam[:n].contiguous())
    w2 = lam[:n * k].view(n, k)
    for bad in (st[:n].cpu(), torch.ones((n, 8), dtype=torch.int32, device="cuda")[:, ::2]):   # a host tensor, a strided one
        with pytest.raises(ValueError):
            cam.create_rays_hero(s[:n].contiguous(), w2, rng_states=bad)
    cam.close()

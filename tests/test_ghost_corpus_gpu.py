"""Ghost rays on the MI355X (zoic_create_ghost_rays_device) over the pinned corpus of machine-made lenses and plates-32, the lens that
fills the tables (tests/lens_losses_corpus.py), after tests/test_ghost_corpus_cpu.py, which holds the host build of csrc/ghost.hpp to
the f64 restatement on the same lenses:

  A  the kernel gives the host build bit for bit on all n x p x 8 words: every pair of ghost_pairs(), bare and with a film wherever
     the media differ, reference_rows of the live spectral records of the frame, the starts from the records' own tries;
  B  the identities of the call on the whole frame (41 472 rows), bit for bit: the chunked launches of more than 32 pairs, every
     column against the p = 1 call of its pair, the reversed pair list, two runs, prefixes, split launches, STRICT against FAST, and
     on the lenses of the most and the fewest interfaces and on plates-32 the frame tiled to 2048 x 256 + 65 rows at p = 1;
  C  dead columns: equal-media pairs, pairs on the stop (at trace index 0 too), invalid pairs, weight-0 rows and rejected wavelengths,
     mixed into live waves and filling whole waves;
  D  an update is seen: the GhostTable in device memory is the updated camera's;
  E  plates-32's forward records are the oracle's, so the start rays are known before any ghost is compared: the first forward run at
     32 interfaces.

Measured on the MI355X (every comparison is exact, so the figures are the sizes of what was compared).  A, per lens, bare and
coated alike -- the film changes no path: rows, pairs, and the census of the n x p records, which is the host build's:

    lens       rows  pairs   traced      miss / clipped / TIR / turned
    triplet-4  3753     6      20 138        0 /   2 380 /      0 /   0
    fisheye-5  3903    55      54 132   49 714 /  99 532 / 10 332 / 955
    mori-6     4001    45      46 807      234 / 132 989 /     15 /   0
    double-3   3858    55     101 913    6 120 /  88 061 / 16 093 /   3
    tessar-5   3802    36      46 106        0 /  90 401 /    365 /   0
    petzval-2  3656    28      41 504        0 /  60 864 /      0 /   0
    mori-4     3911    28      41 304        0 /  68 204 /      0 /   0
    rear-9     3782    21      13 672        0 /  57 980 /  7 714 /  56
    rear-12    3871    21      15 886        0 /  57 789 /  7 616 /   0
    petzval-5  3655    66      70 970       37 / 169 369 /    854 /   0
    plates-32  3876   465   1 263 552        0 / 538 788 /      0 /   0

No word differs on any lens in A, B, C or D.  B: the STRICT and the FAST camera's records agree on every row of every lens
(petzval-5 runs STRICT's kernels).  D: with the exit-pupil LUT the records after updating back are not the first ones -- the LUT is
sampled anew at every update, as the reference's is -- and the call is held to the host build from an oracle camera that has seen the
same updates; without the LUT records and ghosts are bitwise the first ones.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST
from zoic_amd.workloads import ray_rng_states

import ghost_ref as gref
import lens_losses_corpus as lc
import machine_lens_corpus as mc
import host_drivers
from device_cases import bits_f32 as _bits
from differentials_spectral_corpus import WAVE_PERIOD, frame, reference_rows
from fuzz_cameras import _oracle_spectral
from host_drivers import run_ghost_records as run_records, split_ghost as split
from lens_losses_corpus import (BIG, SPLIT, constructed as _constructed, device_camera as _camera, device_inputs as _inputs, device_launch as _launch,
                                device_starts as _starts, record_tries as _tries, same_words as _same, take as _take)
from machine_lens_corpus import PREFIXES
from spectral_ref import BAD, LAMBDA_D32, WAVES

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def driver():
    return host_drivers.ghost()


def _dead(reason, interface=0, leg=0):
    rec = np.zeros(8, np.uint32)
    rec[7] = gref.flag_word(reason, interface, leg)
    return rec


def _census(rec):
    return np.bincount(split(rec)[4].ravel(), minlength=len(gref.REASONS))


# ---- E: the forward precondition of plates-32 ----------------------------------------------------------------------------------------
def test_plates_forward_records_are_the_oracles(gpu, oracle_lib):
    """32 interfaces, STRICT: the d-line records of the whole frame are the oracle's words (flags and all seven floats), the spectral
    call at 587.5618 nm gives them again, and on the rows that carry one of the eight WAVES the spectral records are the oracle's with
    that wavelength's indices written into its lens table.  The tries, and so the start rays, are known before a ghost is compared."""
    name = lc.PLATES
    s, st, lam = (np.array(a) for a in frame())
    cam = _camera(name)
    assert cam.info()["lensCount"] == 32
    R = lc.oracle_frame(oracle_lib, name)
    got = cam.create_rays(s, rng_states=st)
    assert np.array_equal(got["flags"], R["flags"]) and np.array_equal(_bits(got["planes"]), _bits(R["planes"]))
    assert (R["weight"] != 0).sum() >= 40000 and (R["tries"] > 0).sum() >= 1000
    same = cam.create_rays(s, rng_states=st, wavelengths=np.full(len(s), LAMBDA_D32, F32))
    assert np.array_equal(same["flags"], got["flags"]) and np.array_equal(_bits(same["planes"]), _bits(got["planes"]))
    rows = np.flatnonzero(np.arange(len(s)) % WAVE_PERIOD < len(WAVES))
    assert np.isin(lam[rows], WAVES).all() and len(rows) >= 600
    ref, _ = _oracle_spectral(oracle_lib, mc.params(name), cam.dispersion(), s[rows], lam[rows], st[rows], lens_text=lc.LENSES[name].text)
    spec = _launch(name)[rows]
    assert np.array_equal(_bits(spec[:, 0:7].T), _bits(ref["planes"]))
    assert np.array_equal((_bits(spec[:, 7]) & 0xFF).astype(np.uint8), ref["flags"])
    cam.close()


# ---- A: host == device bits, n x p x 8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_kernel_equals_the_host_build(gpu, oracle_lib, driver, name, coated):
    """every word of every pair of ghost_pairs() on reference_rows of the live records (at most 4096, the eight WAVES and the retried
    among them), STRICT, the starts from the records' tries; at least 1000 traced and 1000 dead columns per lens; the device's census of
    reasons is the host's"""
    import torch
    T, S = lc.tables(name), _starts(oracle_lib, name)
    rows = S["rows"]
    assert len(rows) >= 2048 and (_tries(_launch(name))[rows] > 0).sum() >= (200 if name != "mori-4" else 1)
    cam = _camera(name, coated=coated)
    assert np.array_equal(cam.ghost_pairs(), T["pairs"])
    ts, tl, tst, tr = _take(rows, _launch(name)[rows])
    got = cam.create_ghost_rays(ts, tr, T["pairs"], wavelengths=tl, rng_states=tst)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(rows), len(T["pairs"]), 8) and got.dtype == torch.float32
    g = got.cpu().numpy()
    want = run_records(driver, T["L"], T["disp"], S["lam"], S["o"], S["d"], T["pairs"], film=T["film"] if coated else None)
    differ = np.argwhere(_bits(g) != _bits(want))
    assert len(differ) == 0, (name, len(differ), differ[:8].tolist())
    seen, host = _census(g), _census(want)
    print("%-10s %-5s rows %4d pairs %3d  traced %d  miss / clipped / TIR / turned %s" % (
        name, "film" if coated else "bare", len(rows), len(T["pairs"]), seen[0], " / ".join("%d" % v for v in seen[1:5])))
    assert np.array_equal(seen, host)
    assert seen[gref.TRACED] >= 1000 and seen[1:].sum() >= 1000, seen
    cam.close()


# ---- B: identities on the whole frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_pair_list_identities(gpu, name):
    """the whole frame, the library's own streams at a ray_index_base, with the film: the full pair list (two or three chunked launches
    on the lenses with more than 32 pairs, fifteen on plates-32) equals the explicit calls of at most 32 pairs through out=,
    concatenated; every column equals the p = 1 call of its pair; the reversed pair list gives the reversed columns; two runs are
    equal"""
    import torch
    T = lc.tables(name)
    pairs = T["pairs"]
    cam = _camera(name, coated=True)
    ts, _, tl = _inputs()
    n, p, base = len(ts), len(pairs), 1000
    rays = cam.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    full = cam.create_ghost_rays(ts, rays, pairs, wavelengths=tl, ray_index_base=base)
    assert tuple(full.shape) == (n, p, 8)
    parts = []
    for lo in range(0, p, 32):
        out = torch.full((n, len(pairs[lo:lo + 32]), 8), 7.0, device="cuda")
        assert cam.create_ghost_rays(ts, rays, pairs[lo:lo + 32], wavelengths=tl, ray_index_base=base, out=out) is out
        parts.append(out)
    assert _same(torch.cat(parts, 1), full)
    del parts
    for j in range(p):
        one = cam.create_ghost_rays(ts, rays, pairs[j:j + 1], wavelengths=tl, ray_index_base=base)
        assert _same(one[:, 0], full[:, j]), (name, j)
    assert _same(cam.create_ghost_rays(ts, rays, pairs[::-1].copy(), wavelengths=tl, ray_index_base=base), full.flip(1))
    assert _same(cam.create_ghost_rays(ts, rays, pairs, wavelengths=tl, ray_index_base=base), full)
    flags = full[:, :, 7].contiguous().view(torch.int32)
    assert int((flags == 1).sum()) >= 1000 and int((flags != 1).sum()) >= 1000
    torch.cuda.synchronize()
    cam.close()


def _straddling(T):
    """a pair whose leg 1 crosses the stop (the stop at trace index 0: the first pair, whose leg 0 starts on it)"""
    over = [j for j, (a, b) in enumerate(T["pairs"].tolist()) if b < T["stop"] < a]
    return T["pairs"][over[len(over) // 2]:over[len(over) // 2] + 1] if over else T["pairs"][:1]


@pytest.mark.parametrize("name", lc.NAMES)
def test_mode_independent_and_split_launches(gpu, name):
    """A STRICT and a FAST camera agree bit for bit wherever their records' weight and flag words agree: on at least 0.99 of the rows
    where FAST has a kernel of its own, on every row where it runs STRICT's (the shares of the spectral-differentials corpus test).
    Prefixes of 1, 63, 64 and 65 rows and a split at [0, 1, 64, 5037, n] with ray_index_base moved along equal the one launch; on the
    lenses of the most and the fewest interfaces and on plates-32 so does the frame tiled to 2048 x 256 + 65 rows at p = 1 with a pair
    that straddles the stop (samples, streams and wavelengths tiled alike)."""
    import torch
    T = lc.tables(name)
    pairs = T["pairs"][:: -(-len(T["pairs"]) // 32)]              # at most 32 of them, spread over the list
    assert 1 <= len(pairs) <= 32
    ts, _, tl = _inputs()
    n, base = len(ts), 1000
    a = _camera(name, coated=True)
    b = _camera(name, precision=PRECISION_FAST, coated=True)
    ra = a.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    rb = b.create_rays(ts, wavelengths=tl, ray_index_base=base)["rays"]
    ga = a.create_ghost_rays(ts, ra, pairs, wavelengths=tl, ray_index_base=base)
    gb = b.create_ghost_rays(ts, rb, pairs, wavelengths=tl, ray_index_base=base)
    same = (ra[:, 6:8].contiguous().view(torch.int32) == rb[:, 6:8].contiguous().view(torch.int32)).all(1)
    share = float(same.float().mean())
    print("%-10s fastRunsStrict %s, records agree on %.5f of the rows" % (name, bool(b.info()["fastRunsStrict"]), share))
    assert share == 1.0 if b.info()["fastRunsStrict"] else share >= 0.99
    assert _same(ga[same], gb[same])
    b.close()

    def part(lo, hi):
        return a.create_ghost_rays(ts[lo:hi].contiguous(), ra[lo:hi].contiguous(), pairs, wavelengths=tl[lo:hi].contiguous(), ray_index_base=base + lo)
    for m in PREFIXES:
        assert _same(part(0, m), ga[:m]), m
    assert _same(torch.cat([part(lo, hi) for lo, hi in zip(SPLIT, SPLIT[1:] + [n])]), ga)
    if name in mc.LARGE_BATCH or name == lc.PLATES:
        pair = _straddling(T)
        assert T["stop"] > 0 and pair[0, 1] < T["stop"] < pair[0, 0]
        small = a.create_ghost_rays(ts, ra, pair, wavelengths=tl, ray_index_base=base)
        reps = -(-BIG // n)
        st = torch.from_numpy(ray_rng_states(n, seed=1, ray_index_base=base).view(np.int32)).cuda()
        big_s, big_l, big_st = ts.repeat(reps, 1)[:BIG].contiguous(), tl.repeat(reps)[:BIG].contiguous(), st.repeat(reps, 1)[:BIG].contiguous()
        rr = a.create_rays(big_s, wavelengths=big_l, rng_states=big_st)["rays"]
        assert _same(rr, ra.repeat(reps, 1)[:BIG])
        gg = a.create_ghost_rays(big_s, rr, pair, wavelengths=big_l, rng_states=big_st)
        assert tuple(gg.shape) == (BIG, 1, 8) and _same(gg, small.repeat(reps, 1, 1)[:BIG])
        assert int((small[:, 0, 7].contiguous().view(torch.int32) == 1).sum()) >= 100
    torch.cuda.synchronize()
    a.close()


# ---- C: dead columns ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.NAMES)
def test_dead_columns(gpu, oracle_lib, driver, name):
    """reference_rows of the live records and up to 200 of the forward call's own weight-0 rows between them (some lenses of the corpus
    lose none of the frame's samples); pairs on an interface between
    equal media (fisheye-5, petzval-2), pairs on the stop (mori-6 and mori-4: every pair (a, 0)), invalid pairs; records whose weight is
    set to 0 and wavelengths outside [360, 830] and NaN, single lanes of live waves and whole waves: the exact dead record, +0.0 and
    the documented flag word, and every word equal to the host build's"""
    import torch
    T, S = lc.tables(name), _starts(oracle_lib, name)
    rays = _launch(name)
    count, stop = T["count"], T["stop"]
    valid = _straddling(T)[0]
    a, b = int(valid[0]), int(valid[1])
    cases = _constructed(name)                                       # (a, b, NO_REFLECTION, interface, leg) away from a middle stop
    ok = [i for i in range(count) if i != stop and i not in T["equal"]]
    if 0 < stop:
        cases += [(max(ok), stop, gref.NO_REFLECTION, stop, 1)]
        if stop < count - 1:
            cases += [(stop, min(ok), gref.NO_REFLECTION, stop, 0)]
    invalid = [(a, a), (b, a), (count, 0), (200, 100)]
    pairs = np.array([(a, b)] + invalid + [c[:2] for c in cases][:26] + [T["pairs"][-1]], np.int64)
    cases = cases[:26]
    assert len(pairs) <= 32
    dead_rows = mc.strided(np.flatnonzero(rays[:, 6] == 0), 200)
    rows = np.sort(np.concatenate([S["rows"], dead_rows]))
    n = len(rows)
    at = np.searchsorted(rows, S["rows"])
    o, d = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    o[at], d[at] = S["o"], S["d"]
    r = np.array(rays[rows])
    lam = np.array(frame()[2][rows])
    assert (r[:, 6] == 0).sum() == len(dead_rows)
    live = np.flatnonzero(r[:, 6] != 0)
    r[live[live < 64][::9], 6] = 0.0                                 # single lanes of the first wave ...
    r[128:192, 6] = 0.0                                              # ... and a whole wave
    mixed = live[(live >= 320) & (live < 384)][:len(BAD)]
    assert len(mixed) == len(BAD)
    lam[mixed] = BAD                                                 # single lanes of a live wave
    lam[448:512] = np.resize(BAD, 64)                                # a whole wave
    assert (r[448:512, 6] != 0).any() and (r[:64, 6] != 0).any() and (r[:64, 6] == 0).any()
    cam = _camera(name, coated=True)
    ts, _, tst, _ = _take(rows, r)
    got = cam.create_ghost_rays(ts, torch.from_numpy(r).cuda(), pairs, wavelengths=torch.from_numpy(lam).cuda(), rng_states=tst).cpu().numpy()
    want = run_records(driver, T["L"], T["disp"], lam, o, d, pairs, have=r[:, 6] != 0, film=T["film"])
    differ = np.argwhere(_bits(got) != _bits(want))
    assert len(differ) == 0, (name, len(differ), differ[:8].tolist())
    g = _bits(got)
    for j in range(1, 5):
        assert (g[:, j] == _dead(gref.INVALID_PAIR)).all()           # whatever the row holds
    none = r[:, 6] == 0
    with np.errstate(invalid="ignore"):
        bad = ~((lam >= 360) & (lam <= 830))
    others = [0] + list(range(5, len(pairs)))
    for j in others:
        assert (g[none, j] == _dead(gref.NO_START)).all()
        assert (g[~none & bad, j] == _dead(gref.WAVELENGTH)).all()
    assert none[128:192].all() and (~none & bad).sum() >= len(BAD) + 8
    fine = ~none & ~bad
    for k, (_, _, reason, interface, leg) in enumerate(cases):
        assert (g[fine, 5 + k] == _dead(reason, interface, leg)).all(), (name, pairs[5 + k])
    assert len(cases) >= 1 and ((g[fine, 0, 7] & 1) == 1).sum() + ((g[fine, -1, 7] & 1) == 1).sum() >= 100
    cam.close()


# ---- D: an update is seen ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lut", [True, False], ids=["LUT", "noLUT"])
@pytest.mark.parametrize("name", ["triplet-4", "mori-6"])
def test_an_update_is_seen(gpu, oracle_lib, driver, name, lut):
    """after update(fStop = 2 x) and fresh records the call equals the host build on the updated camera's tables, whose stop has a
    smaller housing2, and differs from the first result; on triplet-4, whose stop lies in the middle, it also differs from the host
    build on the OLD tables from the new starts on a pair whose leg 1 crosses the stop, with more ghosts clipped there: the kernel
    reads the GhostTable the update uploaded.  After updating back the tables are bitwise the first ones and the call equals the host
    build on them.  Without the exit-pupil LUT records and ghosts are then bitwise the first ones; with it they are not, by design: the
    LUT is sampled anew at every update from a generator that runs on (as the reference's is), so the lens points move, and the host
    build's starts are taken from an oracle camera that has seen the same updates."""
    import torch
    over = dict(kolbSamplingLUT=lut)
    T = lc.tables(name)
    pairs, meets = T["pairs"], _straddling(T)
    j = int(np.flatnonzero((pairs == meets[0]).all(1))[0])
    ts, tst, tl = _inputs()
    cam = _camera(name, coated=True, **over)
    params = dict(T["params"], **over)
    f = float(params["fStop"])

    def run(*history):
        rays = cam.create_rays(ts, wavelengths=tl, rng_states=tst)["rays"]
        r = rays.cpu().numpy()
        rows = reference_rows(np.flatnonzero(r[:, 6] != 0), _tries(r))
        o, d = lc.kolb_starts(oracle_lib, name, rows, _tries(r)[rows], history, **over)
        a, b, c, e = _take(rows, r[rows])
        got = cam.create_ghost_rays(a, e, pairs, wavelengths=b, rng_states=c).cpu().numpy()
        return r, rows, o, d, got
    lam = np.array(frame()[2])
    T1 = lc.tables_of(cam, params)
    assert np.array_equal(_bits(T1["L"]["housing2"]), _bits(T["L"]["housing2"]))
    r1, rows1, o1, d1, got1 = run()
    assert np.array_equal(_bits(got1), _bits(run_records(driver, T["L"], T["disp"], lam[rows1], o1, d1, pairs, film=T["film"])))
    cam.update(**dict(params, fStop=2 * f))
    T2 = lc.tables_of(cam, dict(params, fStop=2 * f))
    assert T2["L"]["housing2"][T["stop"]] < T["L"]["housing2"][T["stop"]] and np.array_equal(T2["pairs"], pairs)
    assert np.array_equal(np.delete(T2["L"]["housing2"], T["stop"]), np.delete(T["L"]["housing2"], T["stop"]))
    r2, rows2, o2, d2, got2 = run(dict(fStop=2 * f))
    new = run_records(driver, T2["L"], T2["disp"], lam[rows2], o2, d2, pairs, film=T["film"])
    old = run_records(driver, T["L"], T["disp"], lam[rows2], o2, d2, pairs, film=T["film"])
    assert np.array_equal(_bits(got2), _bits(new))
    assert not (np.array_equal(rows1, rows2) and np.array_equal(_bits(got1), _bits(got2)))
    if T["stop"] > 0:     # (a stop at trace index 0 is crossed on leg 0 only, where the ghost still is the record's own path)
        stop_clips = lambda rec: int(((split(rec)[4] == gref.CLIPPED) & (split(rec)[5] == T["stop"])).sum())     # noqa: E731
        assert not np.array_equal(_bits(got2[:, j]), _bits(old[:, j])) and stop_clips(got2[:, j]) > stop_clips(old[:, j])
    cam.update(**params)
    T3 = lc.tables_of(cam, params)
    for k in ("radius", "thickness", "aperture", "vertex", "housing2"):
        assert np.array_equal(_bits(T3["L"][k]), _bits(T["L"][k])), k
    r3, rows3, o3, d3, got3 = run(dict(fStop=2 * f), dict(fStop=f))
    assert np.array_equal(_bits(got3), _bits(run_records(driver, T["L"], T["disp"], lam[rows3], o3, d3, pairs, film=T["film"])))
    if not lut:
        assert np.array_equal(_bits(r3), _bits(r1)) and np.array_equal(rows3, rows1) and np.array_equal(_bits(got3), _bits(got1))
    torch.cuda.synchronize()
    cam.close()

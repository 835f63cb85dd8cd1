"""Hero-wavelength rays on the MI355X against a CPU reference of the whole call (tests/hero_ref.py, checked on its own by
tests/test_hero_cpu.py): STRICT equals hero_reference in all 8 words of all n k records (NaN equal to NaN) and in the counters, with
no tolerance and no row left out -- on the shipped cameras with and without the exit-pupil LUT, with exposure control and a bokeh image,
and on the ten lenses of the pinned corpus; at k = 2, 4 and 8; on short prefixes; on hostile samples and wavelengths with every
rejection pattern forced into known rows; under a permutation of the rows and beside hostile neighbours; and past the grid's first
pass (the second chunk of a wave, the thin-lens copy's second stride).  FAST is held to the same reference by the project's own flip
and direction bounds.

Wavelengths come from hero_cases.palette: one of nine valid values per (row, column), so neighbouring lanes trace at different
wavelengths in the same trace stage."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT
from zoic_amd.workloads import camera_params

import hero_cases as hr
from fuzz_cameras import DIR_RMSE_TOL, FLIP_TOL, HOSTILE_SAMPLES, LAMBDA_EDGES, LAMBDA_HOSTILE, WAVES

pytestmark = pytest.mark.gpu

N, LOST, REJECTED = hr.N, hr.LOST, hr.REJECTED
MODES = [PRECISION_STRICT, PRECISION_FAST]
MODE_IDS = ["strict", "fast"]
assert np.array_equal(hr.WAVES, WAVES)      # the palette is the spectral fuzz's


def _run(name, s, lam, st, precision=PRECISION_STRICT):
    """(words (n, k, 8) uint32, counter deltas) of one create_rays_hero call on a fresh camera"""
    cam = hr.spec(name).camera(precision=precision)
    before = cam.counters()
    got = cam.create_rays_hero(np.array(s), np.array(lam), rng_states=np.array(st))      # copies: the cached inputs are read-only
    after = cam.counters()
    cam.close()
    return hr.words_of(got), {k: after[k] - before[k] for k in after}


def _assert_equals(got, ref, what=""):
    same = hr.same_words(got, ref)
    bad = np.argwhere(~same)
    assert same.all(), (what, len(bad), bad[:8].tolist(), got[~same][:2].tolist(), ref[~same][:2].tolist())


# ---- 1: every camera ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.CAMERAS)
def test_strict_equals_the_reference(oracle_lib, name):
    s, lam, st, ref, counters, _ = hr.reference(oracle_lib, name)
    got, c = _run(name, s, lam, st)
    _assert_equals(got, ref, name)
    assert c == counters, (name, c, counters)
    # the families this batch exercised on the device are the pinned ones
    census = hr.census(got)
    assert census == {f: v for f, v in hr.CENSUS[name].items() if f in census}, (name, census)
    if "exposure" in name:   # the companions carry the hero's weight, and it is not 1
        w = got[:, :, 6].view(np.float32)
        through = (got[:, 1:, 7] & LOST) == 0
        assert through.any() and (np.broadcast_to(w[:, :1], through.shape)[through] == w[:, 1:][through]).all()
        assert (w[:, 1:][through] != 1.0).all()


# ---- 2: shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 8])          # k = 4 is test_strict_equals_the_reference
@pytest.mark.parametrize("name", hr.SHAPES_CAMERAS)
def test_two_and_eight_wavelengths(oracle_lib, name, k):
    s, lam, st, ref, counters, _ = hr.reference(oracle_lib, name, k=k)
    got, c = _run(name, s, lam, st)
    assert got.shape == (N, k, 8)
    _assert_equals(got, ref, (name, k))
    assert c == counters
    assert ((got[:, 1:, 7] & LOST) != 0).any() and ((got[:, 1:, 7] & LOST) == 0).any()


def test_prefixes(oracle_lib):
    """n = 1, 63, 64, 65, 257: a lone lane, a partial wave, a full one, a second wave's first lane, a second chunk's first sample.  C5
    (the most rejections) against the prefix of its reference -- the reference treats every row alone -- and C2 without the LUT
    (half of its heroes retry) against a reference of the prefix itself, counters included."""
    s, lam, st, ref, _, _ = hr.reference(oracle_lib, "C5")
    sp = hr.spec("C2-nolut")
    for n in (1, 63, 64, 65, 257):
        got, c = _run("C5", s[:n], lam[:n], st[:n])
        _assert_equals(got, ref[:n], ("C5", n))
        live = int((got[:, 0, 6].view(np.float32) != 0).sum())
        assert (c["succesRays"], c["vignettedRays"]) == (live, n - live)
        want, cw = hr.hero_reference(oracle_lib, sp.params, sp.dispersion(), s[:n], lam[:n], st[:n])
        got, c = _run("C2-nolut", s[:n], lam[:n], st[:n])
        _assert_equals(got, want, ("C2-nolut", n))
        assert c == cw


# ---- 3: hostile samples and wavelengths ----------------------------------------------------------------------------------------
# rows of the forced patterns, once in the first wave and once far into the batch; each pattern under a live hero (an axial ray) and
# under a hero of weight 0 (a screen sample outside the exit-pupil LUT: a dead pixel)
PATTERN_BLOCKS = (70, 3000)
AXIAL = np.array([0.01, 0.01, 0.55, 0.5], np.float32)
OUTSIDE = np.array([2.9, 1.9, 0.3, 0.7], np.float32)
SPECIAL = np.concatenate([LAMBDA_HOSTILE, LAMBDA_EDGES])


def _hostile_inputs(k=4, seed=23):
    s, lam, st = hr.inputs(N, k, seed)
    s, lam = s.copy(), lam.copy()
    rs = np.random.RandomState(seed)
    hostile = rs.rand(N, 4) < 0.25
    s[hostile] = HOSTILE_SAMPLES[rs.randint(len(HOSTILE_SAMPLES), size=int(hostile.sum()))]
    odd = rs.rand(N, k) < 0.15                                  # in every column
    lam[odd] = SPECIAL[rs.randint(len(SPECIAL), size=int(odd.sum()))]
    good = hr.palette(N, k, seed + 9)
    rows = {}
    for b in PATTERN_BLOCKS:
        lam[b:b + 10] = good[b:b + 10]
        s[b:b + 10:2], s[b + 1:b + 10:2] = AXIAL, OUTSIDE         # even offsets live, odd ones dead
        for dead in (0, 1):
            lam[b + dead, 0] = SPECIAL[(b + dead) % len(LAMBDA_HOSTILE)]               # a bad hero
            lam[b + 2 + dead, 1:3] = [np.inf, 0.0]                                     # two adjacent bad companions
            lam[b + 4 + dead, k - 1] = 830.1                                           # a bad last column
            lam[b + 6 + dead, 1:] = np.nan                                             # all companions bad
            lam[b + 8 + dead, 2] = -500.0                                              # one bad companion (under a dead hero: the issue's case)
        rows[b] = np.arange(b, b + 10)
    return s, lam, st, rows


@pytest.mark.parametrize("name", hr.HOSTILE_CAMERAS)
def test_hostile_batch(oracle_lib, name):
    k = 4
    sp = hr.spec(name)
    s, lam, st, rows = _hostile_inputs(k)
    ok = hr.valid(lam)
    ref, counters = hr.hero_reference(oracle_lib, sp.params, sp.dispersion(), s, lam, st, lens_text=sp.text)
    # the inputs are what they are meant to be: the pattern rows' heroes live and dead in turn, every kind of record present
    w_ref = ref[:, :, 6].view(np.float32)
    for b, r in rows.items():
        assert (w_ref[r[2::2], 0] != 0).all() and (w_ref[r[3::2], 0] == 0).all() and (ref[r[:2], :, 7] == REJECTED).all(), (name, b)
    assert (~ok[:, 0]).sum() >= 64 and (ok[:, 0, None] & ~ok[:, 1:]).sum() >= 64
    assert np.isnan(ref[:, 0, :7].view(np.float32)).any(1).sum() >= 16                  # hostile samples made NaN heroes
    got, c = _run(name, s, lam, st)
    _assert_equals(got, ref, name)
    assert c == counters, (name, c, counters)
    # FAST: legal try counts, the same rejected records, companions in the two legal forms only
    fast, _ = _run(name, s, lam, st, PRECISION_FAST)
    rejected = ref[:, :, 7] == REJECTED
    assert np.array_equal(fast[:, :, 7] == REJECTED, rejected) and not fast[rejected][:, :7].any()
    hero = fast[:, 0, 7]
    rows_ok = ok[:, 0]
    assert (((hero[rows_ok] >> 1) & 31) <= 26).all() and (hero[rows_ok] & ~np.uint32(0x7f) == 0).all()
    comp = ~rejected[:, 1:]
    f = fast[:, 1:, 7][comp]
    hf = np.broadcast_to(hero[:, None], comp.shape)[comp]
    lost = f == (hf | LOST)
    assert (lost | (f == hf)).all()
    assert not fast[:, 1:][comp][lost][:, :7].any()                                     # a lost record is all zeros
    hw = np.broadcast_to(fast[:, :1, 6], comp.shape)[comp]
    assert np.array_equal(fast[:, 1:, 6][comp][~lost], hw[~lost])                       # one that came through carries the hero's weight
    assert lost[hw.view(np.float32) == 0].all()                                         # no start, no companion


# ---- 4: a row does not depend on its neighbours ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES, ids=MODE_IDS)
def test_rows_permuted(oracle_lib, precision):
    s, lam, st, ref, _, _ = hr.reference(oracle_lib, "rear-9")       # the most lost companions and retried heroes
    base, cb = _run("rear-9", s, lam, st, precision)
    if precision == PRECISION_STRICT:
        _assert_equals(base, ref)
    perm = np.random.RandomState(41).permutation(N)
    got, c = _run("rear-9", s[perm], lam[perm], st[perm], precision)
    assert np.array_equal(got, base[perm]), int((got != base[perm]).any((1, 2)).sum())
    assert c == cb


@pytest.mark.parametrize("precision", MODES, ids=MODE_IDS)
def test_rows_beside_hostile_neighbours(oracle_lib, precision):
    """even rows hostile samples, samples of weight 0 and rejected wavelengths; the odd rows give what they give alone"""
    s, lam, st, rows = _hostile_inputs()
    good_s, good_lam, good_st = hr.inputs(N, 4)
    s[1::2], lam[1::2], st = good_s[1::2], good_lam[1::2], good_st
    s[0::4] = OUTSIDE
    alone, _ = _run("C5", s[1::2], lam[1::2], st[1::2], precision)
    mixed, _ = _run("C5", s, lam, st, precision)
    assert np.array_equal(mixed[1::2], alone), int((mixed[1::2] != alone).any((1, 2)).sum())
    if precision == PRECISION_STRICT:
        _assert_equals(alone, hr.reference(oracle_lib, "C5")[3][1::2])
    assert (mixed[0::4, 0, 6] == 0).all()


# ---- 5: past the grid's first pass ---------------------------------------------------------------------------------------------
# mirrored from zoic_amd/csrc/device_pass.hpp and spectral.hip: kPassGridCap blocks of kPassBlock threads; a wave of kolb_spectral_kernel<FAST, HERO> claims
# kSpecChunk samples at a time, a thread of hero_replicate_kernel one row per stride
HERO_GRID_CAP, HERO_BLOCK, HERO_CHUNK = 2048, 256, 256
KOLB_FIRST_PASS = HERO_GRID_CAP * (HERO_BLOCK // 64) * HERO_CHUNK      # 2 097 152 samples
THIN_FIRST_PASS = HERO_GRID_CAP * HERO_BLOCK                           # 524 288 rows


def _tiled(cam, s, lam, st, n):
    """(the 4096-row block's result downloaded, whether the n-row call on the block tiled along the rows equals the block's result
    tiled) -- the comparison stays on the device"""
    import torch
    dev = torch.device("cuda", 0)
    bs, bl = torch.from_numpy(np.array(s)).to(dev), torch.from_numpy(np.array(lam)).to(dev)      # copies: the cached inputs are read-only
    bst = torch.from_numpy(np.array(st).view(np.int32)).to(dev)
    block = cam.create_rays_hero(bs, bl, rng_states=bst)["rays"].clone()
    idx = torch.arange(n, device=dev) % len(s)
    big = cam.create_rays_hero(bs[idx].contiguous(), bl[idx].contiguous(), rng_states=bst[idx].contiguous())["rays"]
    same = torch.equal(big.view(torch.int32), block[idx].view(torch.int32))
    torch.cuda.synchronize(dev)
    return block.cpu().numpy().view(np.uint32), same


def test_second_chunk_of_a_wave(oracle_lib):
    n, k = KOLB_FIRST_PASS + 257, 2
    assert n == 2097152 + 257 and n > KOLB_FIRST_PASS           # wave 0 comes back for the chunk at 2 097 152, one sample into its second wave-row
    s, lam, st, ref, _, _ = hr.reference(oracle_lib, "C5", k=k)
    cam = hr.spec("C5").camera()
    before = cam.counters()
    block, same = _tiled(cam, s, lam, st, n)
    after = cam.counters()
    cam.close()
    _assert_equals(block, ref)
    assert same
    live = int((ref[:, 0, 6].view(np.float32) != 0).sum())
    full, rest = divmod(n, N)
    live_rest = int((ref[:rest, 0, 6].view(np.float32) != 0).sum())
    assert after["succesRays"] - before["succesRays"] == (full + 1) * live + live_rest       # the block's own call, then the tiles
    assert after["vignettedRays"] - before["vignettedRays"] == (full + 1) * (N - live) + rest - live_rest


def test_second_stride_of_the_thin_lens_copy(oracle_lib):
    n, k = THIN_FIRST_PASS + 1, 2
    assert n == 524289 and n > THIN_FIRST_PASS
    from zoic_amd import ZoicCamera
    p = dict(camera_params("C1"), opticalVignettingDistance=5.0)      # the thin lens with its rejection loop
    s, lam, st = hr.inputs(N, k)
    lam = lam.copy()
    lam[5::64, 0], lam[9::64, 1] = np.nan, 831.0                      # rejected rows and columns among them
    ref, counters = hr.hero_reference(oracle_lib, p, None, s, lam, st)
    cam = ZoicCamera(device=0)
    cam.update(**p)
    before = cam.counters()
    block, same = _tiled(cam, s, lam, st, n)
    after = cam.counters()
    cam.close()
    _assert_equals(block, ref)
    # the copy kernel takes back what the thin-lens kernel counted for a rejected hero: the block's own call, then the tiles
    counted = ref[:, 0, 7] != REJECTED
    live = counted & (ref[:, 0, 6] != 0)
    assert (counters["succesRays"], counters["vignettedRays"]) == (int(live.sum()), int((counted & ~live).sum())) and (~counted).sum() >= 64
    full, rest = divmod(n, N)
    assert {key: after[key] - before[key] for key in after} == dict(
        succesRays=(full + 1) * int(live.sum()) + int(live[:rest].sum()),
        vignettedRays=(full + 1) * int((counted & ~live).sum()) + int((counted & ~live)[:rest].sum()), totalInternalReflection=0)
    assert (ref[:, 0, 6].view(np.float32) == 0).any() and (ref[:, 0, 6].view(np.float32) != 0).any()
    assert same


# ---- 6: FAST against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.FAST_CAMERAS)
def test_fast_against_the_reference(oracle_lib, name):
    """rows whose FAST hero has the reference's flags started where the reference's hero did (the start is computed in the reference's
    arithmetic in both modes): there the companions' lost / through decisions differ in at most 20 x FLIP_TOL of them
    (test_spectral_fuzz_gpu's bound at this batch size) and the directions of those that agree and live are within DIR_RMSE_TOL"""
    n, k = 8192, 4
    s, lam, st, ref, _, _ = hr.reference(oracle_lib, name, n=n, k=k)
    fast, _ = _run(name, s, lam, st, PRECISION_FAST)
    cam = hr.spec(name).camera(precision=PRECISION_FAST)
    assert not cam.info()["fastRunsStrict"]
    cam.close()
    rows = (fast[:, 0, 7] == ref[:, 0, 7]) & (ref[:, 0, 6] != 0)
    assert rows.sum() >= 0.95 * (ref[:, 0, 6] != 0).sum()
    a_lost, b_lost = (ref[rows, 1:, 7] & LOST) != 0, (fast[rows, 1:, 7] & LOST) != 0
    flip = float((a_lost != b_lost).mean())
    both = ~a_lost & ~b_lost
    da = ref[rows, 1:, 3:6].view(np.float32)[both].astype(np.float64)
    db = fast[rows, 1:, 3:6].view(np.float32)[both].astype(np.float64)
    finite = np.isfinite(da).all(1)
    rmse = float(np.sqrt(((da[finite] - db[finite]) ** 2).sum(1).mean()))
    print("%s: %d of %d live heroes with the reference's flags, %d companions: flip share %.3g (bound %.3g), direction RMSE %.3g (bound %.3g) over %d"
          % (name, rows.sum(), (ref[:, 0, 6] != 0).sum(), a_lost.size, flip, 20 * FLIP_TOL, rmse, DIR_RMSE_TOL, finite.sum()))
    assert flip < 20 * FLIP_TOL, (name, flip)
    assert finite.sum() > 1000 and rmse < DIR_RMSE_TOL, (name, rmse)
    assert not np.array_equal(fast[rows, 1:][both], ref[rows, 1:][both])                # FAST is not the STRICT kernel

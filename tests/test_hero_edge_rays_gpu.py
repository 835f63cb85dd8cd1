"""Hero companions and their transmittance on guarded clip edges (tests/hero_edge_rays.py), on the MI355X.

csrc/spectral.hip promises that in the FAST modes every clip decision is a FAST one outside its band or a STRICT one, hero tries and
companions alike, and csrc/transmittance.hpp builds on it: a path without transmittance is possible only for records of the unchecked
FAST mode.  Random rows reach a guard band for 0.001 ... 2 % of the rays, so the other hero tests bound a flip *fraction*.  Here every
row's COMPANION sits on a clip edge at its own wavelength: a companion whose dl lags a column, that restarts from the wrong saved start
after the STRICT re-trace, or whose band test is skipped flips here, and must not.

STRICT equals hero_ref.hero_reference in all 8 words of all n k records and in the counters, with the edge column second of two, last
of eight and in the middle of eight.  FAST decides every guarded companion as the reference does (zero flips), leaves every hero where
the reference has it, writes the two legal record forms only and gives the edge column the same bits wherever it stands.  In both
modes a prefix of the rows and the rows interleaved with retrying heroes give what the batch gives.  The transmittance pass over the
same records equals the host build bit for bit and is > 0 exactly where the record has weight."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT

import edge_rays as E
import hero_cases as hr
import hero_edge_rays as H
import host_drivers
import transmittance_cases as TC
from device_cases import bits_f32 as _bits
from fuzz_cameras import DIR_RMSE_TOL
from spectral_ref import spectral_iors

pytestmark = pytest.mark.gpu

LOST = hr.LOST
SHAPES = [(2, 1), (8, 7), (8, 3)]          # (k, the edge column): second of two, last of eight, in the middle of eight
MODES = [PRECISION_STRICT, PRECISION_FAST]
MODE_IDS = ["strict", "fast"]
PREFIXES = (1, 63, 64, 65)
LOSS_CAMERAS = ["C2", "rear-9", "mori-6"]  # the transmittance pass: a shipped lens, the near-hemispherical rear element, the stop at trace index 0
# FAST heroes that do not end where the reference's do: {camera: rows}.  Only an unguarded decision of the hero's own first try (TIR,
# a sphere miss: DESIGN 4.3) explains one; none was found.
HERO_FINDINGS = {}


@pytest.fixture(scope="module")
def driver():
    return host_drivers.transmittance()


def _call(cam, s, lam, st):
    """(words (n, k, 8) uint32, counter deltas) of one create_rays_hero call"""
    before = cam.counters()
    got = cam.create_rays_hero(np.array(s), np.array(lam), rng_states=np.array(st))      # copies: the cached inputs are read-only
    after = cam.counters()
    return hr.words_of(got), {key: after[key] - before[key] for key in after}


def _assert_equals(got, ref, what):
    same = hr.same_words(got, ref)
    bad = np.argwhere(~same)
    assert same.all(), (what, len(bad), bad[:8].tolist(), got[~same][:2].tolist(), ref[~same][:2].tolist())


def _hero_labels(oracle_lib, ce, starts, rows):
    """(row, label, |margin|) of heroes: the decision of the f64 restatement (edge_rays.margins at the hero's index table) that lies
    closest to its threshold along the hero's first try"""
    out = []
    disp = ce["dispersion"]
    for h in np.unique(ce["hero"][rows]):
        r = rows[ce["hero"][rows] == h]
        oc = E.oracle_camera(oracle_lib, ce["p"], ce["lens_text"], ior=spectral_iors(disp["ior_d"], disp["cauchy_b"], h))
        info = oc.lens_table()
        oc.close()
        kinds = dict(zip(("housing", "miss", "tir"), E.margins(info, starts[r, 0:3], starts[r, 3:6])))
        for j, row in enumerate(r):
            m, kind, i = min((abs(float(v)), kind, i) for kind, a in kinds.items() for i, v in enumerate(a[j]) if np.isfinite(v))
            out.append((int(row), "%s(%d)" % (kind, i), m))
    return out


# ---- STRICT -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.CAMERAS)
def test_strict_equals_the_reference(gpu, oracle_lib, name):
    ce = H.edges(oracle_lib, name)
    cam = H.spec(oracle_lib, name).camera()
    for k, col in SHAPES:
        ref, counters, _ = H.reference(oracle_lib, ce, k, col)
        got, c = _call(cam, ce["samples"], H.lambdas(ce, k, col), ce["states"])
        _assert_equals(got, ref, (name, k, col))
        assert c == counters, (name, k, col, c, counters)
    cam.close()


# ---- FAST ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.CAMERAS)
def test_fast_decides_every_guarded_companion_as_the_reference(gpu, oracle_lib, name):
    ce = H.edges(oracle_lib, name)
    guarded = ce["guarded"]
    n = len(guarded)
    cam = H.spec(oracle_lib, name).camera(precision=PRECISION_FAST)
    assert not cam.info()["fastRunsStrict"], "%s: FAST runs STRICT on a camera it must serve" % name
    fast = {shape: _call(cam, ce["samples"], H.lambdas(ce, *shape), ce["states"])[0] for shape in SHAPES}
    cam.close()
    flips, hero_rows, rmse, verdicts = {}, {}, {}, []
    for (k, col), got in fast.items():
        ref, _, det = H.reference(oracle_lib, ce, k, col)
        # decision safety: the edge companion's lost bit on every guarded row
        ref_lost, got_lost = (ref[:, col, 7] & LOST) != 0, (got[:, col, 7] & LOST) != 0
        bad = np.nonzero((ref_lost != got_lost) & guarded)[0]
        flips[(k, col)] = len(bad)
        if len(bad):
            labs = ce["labels"]
            verdicts.append((name, "k = %d, column %d: FAST flips %d guarded companions" % (k, col, len(bad)),
                             {str(v): int((labs[bad] == v).sum()) for v in np.unique(labs[bad])},
                             [(int(i), str(labs[i]), int(ce["offset"][i]), float(ce["margin"][i] / ce["band"][i]), int(ref[i, col, 7]), int(got[i, col, 7]))
                              for i in bad[:8]]))
        # the hero column: the reference's flag word on every row
        differ = np.nonzero(got[:, 0, 7] != ref[:, 0, 7])[0]
        hero_rows[(k, col)] = differ
        if not np.array_equal(differ, np.array(HERO_FINDINGS.get(name, []), dtype=differ.dtype)):
            verdicts.append((name, "k = %d, column %d: %d FAST heroes do not end where the reference's do" % (k, col, len(differ)),
                             differ[:32].tolist(), _hero_labels(oracle_lib, ce, det["starts"], differ[:8])))
        # record form: a lost record is seven zero words with the hero's flags | LOST, one that came through carries the hero's
        # weight and flags
        f = got[:, 1:, 7]
        hf = np.broadcast_to(got[:, :1, 7], f.shape)
        hw = np.broadcast_to(got[:, :1, 6], f.shape)
        lost = (f & LOST) != 0
        assert np.array_equal(f[lost], hf[lost] | LOST) and not got[:, 1:][lost][:, :7].any(), (name, k, col)
        assert np.array_equal(f[~lost], hf[~lost]) and np.array_equal(got[:, 1:, 6][~lost], hw[~lost]), (name, k, col)
        assert (got[:, 0, 6] != 0).all() or len(differ)
        # the through companions' directions
        both = ~ref_lost & ~got_lost
        da = ref[both, col, 3:6].view(np.float32).astype(np.float64)
        db = got[both, col, 3:6].view(np.float32).astype(np.float64)
        rmse[(k, col)] = float(np.sqrt(((da - db) ** 2).sum(1).mean()))
        assert both.sum() >= n // 4, (name, k, col, int(both.sum()))
    print("%s: %d rows, %d guarded | FAST flips on guarded %s | hero-flag differences %s | through companions' direction RMSE %s (bound %.3g)" % (
        name, n, int(guarded.sum()), {"k%d/col%d" % s: v for s, v in flips.items()}, {"k%d/col%d" % s: len(v) for s, v in hero_rows.items()},
        {"k%d/col%d" % s: "%.3g" % v for s, v in rmse.items()}, DIR_RMSE_TOL))
    assert not verdicts, verdicts
    assert max(rmse.values()) < DIR_RMSE_TOL, (name, rmse)
    # independence of the other columns: the same start, the same dl, the same operations
    for k, col in SHAPES[1:]:
        same = (fast[(k, col)][:, col] == fast[(2, 1)][:, 1]).all(1)
        assert same.all(), (name, k, col, int((~same).sum()), np.nonzero(~same)[0][:8].tolist())
    # FAST is not the STRICT kernel.  The edge column itself may well carry the reference's bits on every row: a try inside a band is
    # traced again in STRICT, and every row here lies a few ulps from its edge.  The palette's columns, away from the edge, do not.
    assert not np.array_equal(fast[(8, 7)][:, 1:7], H.reference(oracle_lib, ce, 8, 7)[0][:, 1:7])


# ---- both modes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", H.CAMERAS)
def test_prefixes_and_neighbours(gpu, oracle_lib, name, precision):
    """the first 1, 63, 64 and 65 rows alone give what they give in the batch; and so do the edge rows interleaved one to one with
    the camera's hero_cases.inputs rows, whose heroes retry: hero tries and edge companions share a trace stage"""
    ce = H.edges(oracle_lib, name)
    s, st = ce["samples"], ce["states"]
    n = len(s)
    cam = H.spec(oracle_lib, name).camera(precision=precision)
    for k, col in ((2, 1), (8, 3)):
        lam = H.lambdas(ce, k, col)
        whole, _ = _call(cam, s, lam, st)
        if precision == PRECISION_STRICT:
            _assert_equals(whole, H.reference(oracle_lib, ce, k, col)[0], (name, k, col))
        for m in PREFIXES:
            part, _ = _call(cam, s[:m], lam[:m], st[:m])
            assert np.array_equal(part, whole[:m]), (name, k, col, m, np.argwhere(part != whole[:m])[:8].tolist())
        ns, nl, nst = hr.inputs(n, k, 11, name)
        ms, ml, mst = (np.empty((2 * n,) + a.shape[1:], a.dtype) for a in (s, lam, st))
        for mixed, edge, other in ((ms, s, ns), (ml, lam, nl), (mst, st, nst)):
            mixed[0::2], mixed[1::2] = edge, other
        got, _ = _call(cam, ms, ml, mst)
        assert np.array_equal(got[0::2], whole), (name, k, col, int((got[0::2] != whole).any((1, 2)).sum()))
        retried = (got[1::2, 0, 7] & 1) != 0
        assert retried.sum() >= 64, (name, int(retried.sum()))
    cam.close()


# ---- the transmittance pass over the same records ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("shape", [(2, 1), (8, 7)], ids=["k2", "k8"])
@pytest.mark.parametrize("name", LOSS_CAMERAS)
def test_transmittance_of_companion_edges(gpu, oracle_lib, driver, name, shape, coated, precision):
    """cam.transmittance equals the host build from the recorded starts and the lens's own clip limits bit for bit on every row; T > 0
    exactly where the record has weight and a valid wavelength and +0.0 elsewhere -- on every row of STRICT records, on every guarded
    row of FAST ones (transmittance.hpp, "No path", where it could break: the replay is STRICT arithmetic, the record's decision was
    FAST outside the band)"""
    import torch
    k, col = shape
    ce = H.edges(oracle_lib, name)
    ref, _, det = H.reference(oracle_lib, ce, k, col)
    lam = H.lambdas(ce, k, col)
    cam = TC.coat(H.spec(oracle_lib, name).camera(precision=precision), name, coated)
    ts, tl = torch.from_numpy(np.array(ce["samples"])).cuda(), torch.from_numpy(lam).cuda()
    tst = torch.from_numpy(np.array(ce["states"]).view(np.int32)).cuda()
    rays = cam.create_rays_hero(ts, tl, rng_states=tst)["rays"]
    got = cam.transmittance(ts, rays, wavelengths=tl, rng_states=tst)
    torch.cuda.synchronize()
    assert tuple(got.shape) == lam.shape and got.dtype == torch.float32
    r = rays.cpu().numpy()
    g = got.cpu().numpy()
    cam.close()
    words, w = r.view(np.uint32), r[:, :, 6]
    if precision == PRECISION_STRICT:
        _assert_equals(words, ref, (name, k, col))
    # a hero with the reference's flag word started where the reference's hero did: every row (test_fast_decides_... holds FAST to it)
    known = words[:, 0, 7] == ref[:, 0, 7]
    assert known.all(), (name, np.nonzero(~known)[0][:8].tolist())
    want = TC.expected(driver, name, coated, det["starts"], lam, w)
    assert np.array_equal(_bits(g), _bits(want)), (name, np.argwhere(_bits(g) != _bits(want))[:8].tolist())
    live = (w != 0) & hr.valid(lam)
    assert (g < 1).all() and not _bits(g[~live]).any()
    rows = np.ones(len(g), bool) if precision == PRECISION_STRICT else ce["guarded"]
    dark = np.argwhere(live[rows] & ~(g[rows] > 0))
    assert not len(dark), (name, "records with weight whose replayed path does not pass", len(dark), dark[:8].tolist())
    lost = (words[:, col, 7] & LOST) != 0
    assert lost.sum() >= len(g) // 4 and (~lost).sum() >= len(g) // 4 and not _bits(g[lost, col]).any()

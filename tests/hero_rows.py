"""The rows form of a hero call, for tests/test_hero_rows_cpu.py and tests/test_hero_rows_gpu.py: a plain helper module.

create_rays_hero on samples (n,4), lam (n,k) and states (n,4) gives rays (n,k,8).  Every pass over records that already exist --
ray_differentials, transmittance at k = 1, create_ghost_rays, trace_back and its Jacobian -- takes them as R = n k rows:
row r = i k + j has samples_r = samples[i], states_r = states[i], lam_r = lam[i, j] and rays_r = rays[i, j] (flat()).

rows() adds what the cached reference of the call (hero_cases.reference) says about each row: its eight words, the start of the hero's
accepted try (details["starts"][i]: the companion's own start), its class -- THROUGH (weight != 0), LOST (weight 0: a lost
companion, a companion of a dead hero, a dead hero) or REJECTED (0x80) -- and whether the hero was accepted at a retry.
f64() is the f64 reference of the through companions from those starts at the companions' own wavelengths
(differentials_spectral_ref through differentials_spectral_corpus.reference): nothing of any library output is read there."""
from collections import OrderedDict, namedtuple

import numpy as np

from zoic_amd import THINLENS

import differentials_ref as dref
import differentials_spectral_corpus as dsc
import differentials_spectral_ref as sref
import ghost_ref as gref
import hero_cases as hr
from transmittance_ref import films_where_media_differ, housings

F32 = np.float32
THROUGH, LOST, REJECTED = 0, 1, 2
# case -> (camera of hero_cases, k): the shipped lens with and without the exit-pupil LUT (without it 95 % of the through companions
# belong to retried heroes), the image sampler, the corpus lenses of the fewest and the most interfaces and the one whose stop is the
# first interface, and k = 8 on one camera of hero_cases.SHAPES_CAMERAS
CASES = OrderedDict([("C2", ("C2", 4)), ("C2-nolut", ("C2-nolut", 4)), ("C3-bokeh-V50", ("C3-bokeh-V50", 4)), ("triplet-4", ("triplet-4", 4)),
                     ("fisheye-5", ("fisheye-5", 4)), ("mori-6", ("mori-6", 4)), ("C5-k8", ("C5", 8))])
CORPUS = ["triplet-4", "fisheye-5", "mori-6"]
assert CASES["C5-k8"][0] in hr.SHAPES_CAMERAS
THIN = "C2-thin"                     # C2 with lensModel = THINLENS; the vignetting distance makes its rejection loop run (retried heroes)
PREFIXES = (1, 63, 64, 65)
GHOST_MIN = 1000                     # the fewest traced and the fewest ended ghosts of a camera's pairs (tests/test_ghost_gpu.py's census)
ALL_PAIRS = "C2"                     # the camera that runs all 21 of its pairs; the others run EIGHT spread over their lists


def spec(case):
    if case == THIN:
        return hr.Spec(dict(hr.spec("C2").params, lensModel=THINLENS, opticalVignettingDistance=20.0))
    return hr.spec(CASES[case][0])


def flat(samples, lam, states, rays=None):
    """(samples_r (R,4), lam_r (R,), states_r (R,4) or None, rays_r (R,8) or None) of a hero call's inputs and records: numpy arrays or
    torch tensors alike"""
    n, k = lam.shape
    if isinstance(lam, np.ndarray):
        rep = lambda a: None if a is None else np.repeat(a, k, 0)          # noqa: E731
        return rep(samples), np.ascontiguousarray(lam).reshape(n * k), rep(states), None if rays is None else np.ascontiguousarray(rays).reshape(n * k, 8)
    rep = lambda a: None if a is None else a.repeat_interleave(k, 0).contiguous()   # noqa: E731
    return rep(samples), lam.contiguous().view(n * k), rep(states), None if rays is None else rays.contiguous().view(n * k, 8)


Rows = namedtuple("Rows", "n k samples lam states words samples_r lam_r states_r words_r starts_r hero col cls retried weight through_companions")
_ROWS = {}


def rows(oracle_lib, case):
    """the rows form of hero_cases.reference(camera, k = the case's) with what the reference says of every row; cached, not to be written to:
      n, k, samples (n,4), lam (n,k), states (n,4), words (n,k,8)        the call
      samples_r, lam_r, states_r, words_r (R,8)                          its rows
      starts_r (R,6)     the start of the hero's accepted try (zeros where the hero has none)
      hero, col (R,)     i and j of row r
      cls (R,)           THROUGH, LOST or REJECTED, from the reference's words
      retried (R,) bool  the hero was accepted at a try > 0
      weight (R,) f32    the reference's weight
      through_companions the rows with col >= 1 and cls == THROUGH"""
    if case not in _ROWS:
        name, k = CASES[case]
        s, lam, st, words, _, det = hr.reference(oracle_lib, name, k=k)
        n = len(s)
        s_r, lam_r, st_r, words_r = flat(s, lam, st, words)
        hero, col = np.repeat(np.arange(n), k), np.tile(np.arange(k), n)
        weight = words_r[:, 6].copy().view(F32)
        cls = np.where(words_r[:, 7] == hr.REJECTED, REJECTED, np.where(weight != 0, THROUGH, LOST))
        retried = np.repeat(((words[:, 0, 7] >> 1) & 31) > 0, k) & (cls != REJECTED)
        R = Rows(n, k, s, lam, st, words, s_r, lam_r, st_r, words_r, np.repeat(det["starts"], k, 0), hero, col, cls, retried, weight,
                 np.flatnonzero((col >= 1) & (cls == THROUGH)))
        for a in R:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ROWS[case] = R
    return _ROWS[case]


Tables = namedtuple("Tables", "info disp surf hs housing2 lens film pairs")
_TABLES = {}


def tables(case):
    """of a tables-only camera: info, dispersion, surfaces (differentials_ref.surfaces), halfSensor, housing2, the ghost geometry
    (ghost_ref.lens), the films of the coated runs in trace order, and the pairs (p,2) the case's ghost calls run"""
    if case not in _TABLES:
        sp = spec(case)
        cam = sp.camera(device=-1)
        info, disp, every = cam.info(), cam.dispersion(), cam.ghost_pairs()
        cam.close()
        hs = F32(F32(sp.params["sensorWidth"]) * F32(0.5))
        if case == THIN:                                                   # a lens without interfaces: no tables, and it lists no pairs
            _TABLES[case] = Tables(info, disp, None, hs, None, None, None, np.array([(3, 1), (1, 3), (7, 0)], np.int32))
        else:
            pairs = every if case == ALL_PAIRS else every[np.linspace(0, len(every) - 1, 8).round().astype(int)]
            assert case != ALL_PAIRS or len(every) == 21
            _TABLES[case] = Tables(info, disp, dref.surfaces(info), hs, housings(info), gref.lens(info), films_where_media_differ(disp), pairs)
    return _TABLES[case]


def coat(cam, case, coated):
    if coated:
        nc, l0 = tables(case).film
        cam.set_coatings(nc[::-1], l0[::-1])      # file order
    return cam


_F64 = {}


def f64(oracle_lib, case):
    """The f64 reference of the case's through companions, from the recorded starts at the companions' wavelengths; cached:
      rows       the through companions (indices into the R rows)
      passes     (m,) bool: the f64 trace from the start at the companion's wavelength comes through (sref.passes)
      eo, ed     (m,) the f64 trace's end against the reference's own companion record (relative)
      ref        differentials_spectral_corpus.reference() of the m rows
      good       passes: the rows that are compared; left_out = the share that is not"""
    if case not in _F64:
        R, T = rows(oracle_lib, case), tables(case)
        tc = R.through_companions
        o0, d0, lam = R.starts_r[tc, 0:3], R.starts_r[tc, 3:6], R.lam_r[tc]
        ok = sref.passes(T.surf, sref.cauchy_eta(T.disp, lam), o0, d0)
        ref = dsc.reference(T.surf, T.disp, T.hs, lam, o0, d0)
        ro, rd = ref["end"]
        rec = R.words_r[tc, 0:6].copy().view(F32)
        with np.errstate(all="ignore"):
            eo = np.linalg.norm(-ro - rec[:, 0:3], axis=1) / np.linalg.norm(rec[:, 0:3], axis=1)
            ed = np.linalg.norm(-rd - rec[:, 3:6], axis=1) / np.linalg.norm(rec[:, 3:6], axis=1)
        _F64[case] = dict(rows=tc, passes=ok, good=ok, left_out=float((~ok).mean()), eo=eo, ed=ed, ref=ref, o0=o0, d0=d0, lam=lam,
                          retried=int(R.retried[tc][ok].sum()))
    return _F64[case]


def spectral_bounds_hold(m):
    """tests/test_differentials_spectral_gpu.py's bounds on differentials_spectral_corpus.figures(): screen tangents median <= 1e-5 and
    99.9 % within 1e-3; the wavelength tangent at most 4 x the screen figures against its contributions and against its own size"""
    return bool(m["s_med"] <= 1e-5 and m["s_ok"] >= 0.999 and m["c_med"] <= 4 * m["s_med"] and m["c_tail"] <= 4 * m["s_tail"]
                and m["l_med"] <= 4 * m["s_med"] and m["l_tail"] <= 4 * m["s_tail"])


def ghost_census(records):
    """(traced, ended) of ghost records (..., 8) float32"""
    flags = np.ascontiguousarray(records[..., 7], F32).view(np.uint32)
    return int((flags == 1).sum()), int((flags != 1).sum())

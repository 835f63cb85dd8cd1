"""Shared inputs of the Fresnel-transmittance and ghost-ray corpus tests (tests/test_ghost_corpus_cpu.py, test_ghost_corpus_gpu.py,
test_transmittance_corpus_cpu.py, test_transmittance_corpus_gpu.py): a helper, not a test.

Lenses: the ten of machine_lens_corpus.NAMES and one defined here, plates-32, the only lens of the suite that fills the tables
(kMaxSurfaces = 32): nine weak air-spaced plates in front of fuzz_cameras.CUSTOM_LENS_14, four columns, with V-numbers of its own so
that the wavelength matters.  It is not part of machine_lens_corpus.CORPUS (the backward-path tests do not run it); its text is pinned
by its zlib.crc32 as the corpus is.

Frame, wavelengths and row selection are those of tests/test_differentials_spectral_corpus_cpu.py (frame, reference_rows); starts are
differentials_ref.kolb_start on the records' own tries; tables come from a tables-only camera.  The host builds are compared on all of
reference_rows (at most MAX_HOST) and so is the f64 transmittance, one vectorised pass; the f64 ghost restatement, a pass per pair, runs
on a stride of them (at most MAX_F64; plates-32, with 465 pairs, MAX_F64_PLATES)."""
import zlib

import numpy as np

import differentials_ref as dref
import ghost_ref as gref
import machine_lens_corpus as mc
from fuzz_cameras import ABBE_RANGE, CUSTOM_LENS_14, MachineLens
from test_differentials_spectral_corpus_cpu import frame, reference_rows
from test_transmittance_cpu import films_where_media_differ, housings
from zoic_amd import ZoicCamera

F32 = np.float32
PLATES = "plates-32"
NAMES = list(mc.NAMES) + [PLATES]
MAX_HOST = 4096            # rows of a lens the host builds are run on (reference_rows' own cap)
MAX_F64 = 1024             # ... and the f64 restatements
MAX_F64_PLATES = 128       # plates-32 has 465 pairs: 59 520 ghosts at this many rows


def plates_text(plates=9):
    """`plates` weak air-spaced plates, front first, then CUSTOM_LENS_14: 2 * plates + 14 interfaces"""
    return "".join("%g\t1.0\t%g\t44.0\n%g\t0.5\t0.0\t44.0\n" % (3000 + 100 * k, 1.5 + 0.01 * k, 3000 + 100 * k) for k in range(plates)) + CUSTOM_LENS_14


PLATES_LENS = MachineLens(plates_text(), np.random.RandomState(32).uniform(ABBE_RANGE[0], ABBE_RANGE[1], 32).astype(F32))
PLATES_CRC = 0xa7a98ec8
LENSES = dict(mc.LENSES, **{PLATES: PLATES_LENS})
# interfaces, trace index of the stop, len(ghost_pairs()), the interfaces other than the stop between equal media at the d-line (trace
# order): where an element was dropped or an air row doubled, two air rows meet
SHAPE = {
    "triplet-4": (5, 2, 6, ()),
    "fisheye-5": (14, 5, 55, (6, 9)),
    "mori-6": (11, 0, 45, ()),
    "double-3": (12, 6, 55, ()),
    "tessar-5": (10, 6, 36, ()),
    "petzval-2": (10, 4, 28, (0,)),
    "mori-4": (9, 0, 28, ()),
    "rear-9": (8, 4, 21, ()),
    "rear-12": (8, 4, 21, ()),
    "petzval-5": (13, 6, 66, ()),
    PLATES: (32, 7, 465, ()),
}


def crc(name):
    return zlib.crc32(LENSES[name].text.encode())


def camera(name, device=-1, precision=None, **over):
    """(camera, params) of a lens of NAMES behind machine_lens_corpus.params (`over`: parameters changed): a tables-only camera by
    default"""
    p = dict(mc.params(name), **over)
    cam = ZoicCamera(device=device)
    LENSES[name].load(cam)
    if precision is not None:
        cam.set_precision(precision)
    cam.update(**p)
    return cam, p


def oracle_camera(oracle_lib, name, history=(), **over):
    """an updated OracleCamera behind lens `name` (the caller closes it).  history: parameter changes of further updates, in order --
    the exit-pupil LUT is sampled anew at every update from a generator that runs on, in the reference and in the library alike, so a
    camera's start rays depend on the updates it has seen"""
    oc = oracle_lib.OracleCamera()
    oc.set_lens_text(LENSES[name].text)
    oc.update(**dict(mc.params(name), **over))
    for change in history:
        oc.update(**dict(mc.params(name), **dict(over, **change)))
    return oc


def tables_of(cam, p):
    """what the host drivers and the restatements take, from any updated camera"""
    info, disp = cam.info(), cam.dispersion()
    n1 = disp["ior_d"]
    differ = n1 != np.append(n1[1:], F32(1.0))
    stop = int(info["apertureElement"])
    return dict(params=p, info=info, disp=disp, L=gref.lens(info), surf=dref.surfaces(info), housing2=housings(info),
                film=films_where_media_differ(disp), pairs=cam.ghost_pairs(), count=int(info["lensCount"]), stop=stop,
                equal=tuple(int(i) for i in np.flatnonzero(~differ) if i != stop))


_TABLES = {}


def tables(name):
    """tables_of a tables-only camera behind lens `name`, cached"""
    if name not in _TABLES:
        cam, p = camera(name)
        _TABLES[name] = tables_of(cam, p)
        cam.close()
    return _TABLES[name]


_ORACLE = {}


def oracle_frame(oracle_lib, name):
    """the oracle's d-line records of the frame behind lens `name`, cached and not to be written to: dict of origin (N,3), dir (N,3),
    weight (N,), tries (N,), flags (N,) and the planes as the oracle returns them"""
    if name not in _ORACLE:
        s, st, _ = frame()
        oc = oracle_camera(oracle_lib, name)
        r = oc.create_rays(s, rng_states=st)
        oc.close()
        _ORACLE[name] = dict(origin=r["origin"].T.copy(), dir=r["dir"].T.copy(), weight=r["weight"].copy(), tries=r["tries"].astype(np.int64),
                             flags=r["flags"].copy(), planes=r["planes"].copy())
        for a in _ORACLE[name].values():
            a.setflags(write=False)
    return _ORACLE[name]


def kolb_starts(oracle_lib, name, rows, tries, history=(), **over):
    """(o0, d0) f32 of the frame's rows `rows`, each at its try tries[k]: differentials_ref.kolb_start"""
    s, st, _ = frame()
    oc = oracle_camera(oracle_lib, name, history, **over)
    p = dict(mc.params(name), **dict(over, **(history[-1] if history else {})))
    o0, d0 = dref.kolb_start(oc, p, s[rows], np.asarray(tries, np.int64), st[rows], oracle_lib)
    oc.close()
    return o0, d0


_STARTS = {}


def starts(oracle_lib, name):
    """The CPU tests' starts: reference_rows of the oracle's live d-line records behind lens `name`, their starts and the frame's
    wavelengths: dict of rows, o, d, lam (all of them, at most MAX_HOST) and f64 (indices into them, at most MAX_F64)"""
    if name not in _STARTS:
        R = oracle_frame(oracle_lib, name)
        rows = reference_rows(np.flatnonzero(R["weight"] != 0), R["tries"])
        assert len(rows) <= MAX_HOST
        o, d = kolb_starts(oracle_lib, name, rows, R["tries"][rows])
        _STARTS[name] = dict(rows=rows, o=o, d=d, lam=np.array(frame()[2][rows]), f64=f64_subset(name, len(rows)))
    return _STARTS[name]


def f64_subset(name, n):
    """indices into n rows that get an f64 restatement: a stride, at most MAX_F64 (plates-32: MAX_F64_PLATES)"""
    return mc.strided(np.arange(n), MAX_F64_PLATES if name == PLATES else MAX_F64)

"""Shared inputs of the Fresnel-transmittance and ghost-ray corpus tests (tests/test_ghost_corpus_cpu.py, test_ghost_corpus_gpu.py,
test_transmittance_corpus_cpu.py, test_transmittance_corpus_gpu.py): a helper, not a test.

Lenses: the ten of machine_lens_corpus.NAMES and one defined here, plates-32, the only lens of the suite that fills the tables
(kMaxSurfaces = 32): nine weak air-spaced plates in front of fuzz_cameras.CUSTOM_LENS_14, four columns, with V-numbers of its own so
that the wavelength matters.  It is not part of machine_lens_corpus.CORPUS (the backward-path tests do not run it); its text is pinned
by its zlib.crc32 as the corpus is.

Frame, wavelengths and row selection are those of differentials_spectral_corpus.py (frame, reference_rows); starts are
differentials_ref.kolb_start on the records' own tries; tables come from a tables-only camera.  The host builds are compared on all of
reference_rows (at most MAX_HOST) and so is the f64 transmittance, one vectorised pass; the f64 ghost restatement, a pass per pair, runs
on a stride of them (at most MAX_F64; plates-32, with 465 pairs, MAX_F64_PLATES).

The two GPU files also share what is at the end: a camera on device 0, the frame uploaded once, one STRICT launch per lens and the
starts rebuilt from its records, all cached."""
import zlib

import numpy as np

import differentials_ref as dref
import ghost_ref as gref
import machine_lens_corpus as mc
from device_cases import BIG, bits_f32  # noqa: F401 (BIG: shared by the two GPU files)
from differentials_spectral_corpus import frame, reference_rows
from fuzz_cameras import ABBE_RANGE, CUSTOM_LENS_14, MachineLens
from transmittance_ref import films_where_media_differ, housings
from zoic_amd import PRECISION_STRICT, ZoicCamera

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


def constructed(name):
    """pairs of the lens the pair list leaves out, with the dead record each must give: (a, b, reason, interface, leg)"""
    T = tables(name)
    count, stop, out = T["count"], T["stop"], []
    ok = [i for i in range(count) if i != stop and i not in T["equal"]]
    for e in T["equal"]:
        out += [(e, b, gref.NO_REFLECTION, e, 0) for b in ok if b < e][:2]              # a on the equal-media interface: leg 0
        out += [(a, e, gref.NO_REFLECTION, e, 1) for a in ok if a > e][-2:]             # b on it: leg 1
    if stop == 0:
        out += [(a, 0, gref.NO_REFLECTION, 0, 1) for a in ok]                           # every pair (a, 0)
    return out


# ---- what the two GPU files share ---------------------------------------------------------------------------------------------------
SPLIT = [0, 1, 64, 5037]


def record_tries(rays):
    return ((bits_f32(rays[:, 7]) >> 1) & 31).astype(np.int64)


def device_camera(name, precision=PRECISION_STRICT, coated=False, **over):
    cam, p = camera(name, device=0, precision=precision, **over)
    if coated:
        nc, l0 = tables(name)["film"]
        cam.set_coatings(nc[::-1], l0[::-1])      # file order
    return cam


_INPUTS = []


def device_inputs():
    """the frame on the device: (samples, rng states as int32, wavelengths) tensors, uploaded once and never written to"""
    if not _INPUTS:
        import torch
        s, st, lam = frame()
        _INPUTS.extend([torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(st).view(np.int32)).cuda(), torch.from_numpy(np.array(lam)).cuda()])
    return tuple(_INPUTS)


_LAUNCH = {}


def device_launch(name):
    """One STRICT launch of the frame at its wavelengths behind lens `name`: the records (N, 8) as numpy, not to be written to"""
    if name not in _LAUNCH:
        import torch
        cam = device_camera(name)
        ts, tst, tl = device_inputs()
        rays = cam.create_rays(ts, wavelengths=tl, rng_states=tst)["rays"]
        torch.cuda.synchronize()
        _LAUNCH[name] = rays.cpu().numpy()
        _LAUNCH[name].setflags(write=False)
        cam.close()
    return _LAUNCH[name]


_DEVICE_STARTS = {}


def device_starts(oracle_lib, name):
    """reference_rows of the launch's live records and their starts from the records' own tries: dict of rows, o, d, lam; not to be
    written to"""
    if name not in _DEVICE_STARTS:
        rays = device_launch(name)
        rows = reference_rows(np.flatnonzero(rays[:, 6] != 0), record_tries(rays))
        o, d = kolb_starts(oracle_lib, name, rows, record_tries(rays)[rows])
        _DEVICE_STARTS[name] = dict(rows=rows, o=o, d=d, lam=np.array(frame()[2][rows]))
        for a in _DEVICE_STARTS[name].values():
            a.setflags(write=False)
    return _DEVICE_STARTS[name]


def take(rows, rays):
    """device tensors of the frame's rows `rows`: samples, wavelengths, rng states and the records `rays` (numpy (len(rows), 8))"""
    import torch
    ts, tst, tl = device_inputs()
    idx = torch.from_numpy(np.array(rows, np.int64)).cuda()      # a copy: rows may be a read-only cached array
    return ts[idx].contiguous(), tl[idx].contiguous(), tst[idx].contiguous(), torch.from_numpy(np.array(rays)).cuda()


def same_words(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

"""A pinned corpus of machine-made lenses for the backward paths (tests/test_backward_corpus_cpu.py, tests/test_backward_corpus_gpu.py):
ten prescriptions made by fuzz_cameras.perturbed_prescription(lens, seed, amount, surgery, abbe=True), every one behind the same
camera (fuzz_cameras.EXAMPLE_CAMERA with sensorHeight 2.0 and no bokeh image).  A four-column lens gets its V-numbers through
set_abbe_numbers (MachineLens.load), a five-column one carries them in its V column.

The generated text of each lens is pinned by its zlib.crc32: a generator that drifts changes the corpus, and the measured tables of
the two test files with it, so test_backward_corpus_cpu.py::test_the_corpus_is_the_pinned_one fails first.

ACCURACY lenses are held to the f64 criteria (the reference alone meets the conditions on them, asserted before the library is looked
at) and to the bitwise device-equals-host comparison; BITWISE lenses to the bitwise comparison and to the f64 trace's decisions only:
their grazing rear surfaces (or, for mori-4, a 400 nm projection too close to its bound) make an f32 accuracy bound a statement about
conditioning, not about the kernels; petzval-5 lies outside the geometric domain and every item is refused."""
import zlib
from collections import namedtuple

import numpy as np

from zoic_amd import ZoicCamera

import traceback_cases as tc
from device_cases import records
from fuzz_cameras import EXAMPLE_CAMERA, REAR_ELEMENT_LENS, perturbed_prescription
from reverse_ref import kolb_point_set

F32 = np.float32


def _rear(radius, back):
    return REAR_ELEMENT_LENS.format(r=abs(radius), radius=radius, back=back)


Entry = namedtuple("Entry", "name lens seed amount surgery interfaces crc accuracy")

#       name          prescription                  seed  amount  surgery  interfaces  crc32 of the text  held to the f64 accuracy bounds
CORPUS = [
    Entry("triplet-4", "triplet_f2.5.dat",           4, 0.05, "drop2",    5, 0x865d998b, True),    # the generator's fewest interfaces
    Entry("fisheye-5", "fisheye_muller_f4.0.dat",    5, 0.05, "double2", 14, 0xa8c91fd9, True),    # ... and its most
    Entry("mori-6",    "mori_f2.8.dat",              6, 0.2,  "keep",    11, 0xb3ffc517, True),    # the stop at trace index 0
    Entry("double-3",  "double_gauss_f2.0.dat",      3, 0.1,  "double",  12, 0x891e4331, True),
    Entry("tessar-5",  "tessar_f2.8.dat",            5, 0.05, "double2", 10, 0x31c0f82d, True),    # five-column, with a V column
    Entry("petzval-2", "petzval_f1.25.dat",          2, 0.1,  "drop",    10, 0x0ae36435, True),
    Entry("mori-4",    "mori_f2.8.dat",              4, 0.05, "drop2",    9, 0x3b3fcb30, False),   # the stop at trace index 0
    Entry("rear-9",    _rear(-9.0, 20.0),            0, 0.0,  "keep",     8, 0xfcd3adff, False),   # near-hemispherical rear element
    Entry("rear-12",   _rear(-12.0, 30.0),           0, 0.0,  "keep",     8, 0xc6434b29, False),   # near-hemispherical rear element
    Entry("petzval-5", "petzval_f1.25.dat",          5, 0.05, "double2", 13, 0x0efa0668, False),   # outside the geometric domain
]
BY_NAME = {e.name: e for e in CORPUS}
NAMES = [e.name for e in CORPUS]
ACCURACY = [e.name for e in CORPUS if e.accuracy]
BITWISE = [e.name for e in CORPUS if not e.accuracy]
OUTSIDE = "petzval-5"            # every trace-back kTbOutsideDomain, every projection kRevOutsideDomain
LARGE_BATCH = ("fisheye-5", "triplet-4")   # the most and the fewest interfaces: also run as more than one grid
MAX_RAYS, MAX_POINTS = 8192, 2048          # what a GPU test gives the per-item host calls
PREFIXES = (1, 63, 64, 65)                 # the batch sizes every device-equals-host comparison also runs
GRID_PLUS_ONE = 524289                     # one grid of 2048 x 256 lanes and one item more
EDGE_CAP = 0.02                            # the largest share of a lens's live rays a conditioning rule may leave out

LENSES = {e.name: perturbed_prescription(e.lens, e.seed, e.amount, e.surgery, abbe=True) for e in CORPUS}


def crc(name):
    return zlib.crc32(LENSES[name].text.encode())


def params(name):
    p = {k: v for k, v in EXAMPLE_CAMERA.items() if k != "image"}
    p.update(sensorHeight=2.0, useImage=False, lensDataPath="mem:corpus_%s" % name)
    return p


def camera(name, device=-1, precision=None):
    """(camera, params) of a corpus lens: a tables-only camera by default"""
    p = params(name)
    cam = ZoicCamera(device=device)
    LENSES[name].load(cam)
    if precision is not None:
        cam.set_precision(precision)
    cam.update(**p)
    return cam, p


_RECORDS = {}


def oracle_camera(oracle_lib, name):
    """an updated OracleCamera behind lens `name` (the caller closes it)"""
    oc = oracle_lib.OracleCamera()
    oc.set_lens_text(LENSES[name].text)
    oc.update(**params(name))
    return oc


def _oracle_frame(oracle_lib, name):
    if name not in _RECORDS:
        s, st = tc.frame_samples()
        oc = oracle_camera(oracle_lib, name)
        r = oc.create_rays(s, rng_states=st)
        _RECORDS[name] = s, r["origin"].T.copy(), r["dir"].T.copy(), r["weight"].copy(), r["tries"].astype(np.int64)
        oc.close()
        for a in _RECORDS[name]:
            a.setflags(write=False)
    return _RECORDS[name]


def oracle_records(oracle_lib, name):
    """the oracle's forward records of the frame tc.W x tc.H x tc.SPP behind lens `name` (the STRICT kernel's bits), cached and not to
    be written to: samples (N,4), origin (N,3), dir (N,3), weight (N,)"""
    return _oracle_frame(oracle_lib, name)[:4]


def oracle_tries(oracle_lib, name):
    """(N,) the try each of oracle_records' rays was accepted at (0: the sample's own lens point)"""
    return _oracle_frame(oracle_lib, name)[4]


_POINTS = {}


def point_set(name):
    """reverse_ref.kolb_point_set of a corpus lens, cached: (points (m,3) f32, samples (m,2), depth index (m,)); empty outside the domain"""
    if name not in _POINTS:
        if name == OUTSIDE:
            _POINTS[name] = np.zeros((0, 3), F32), np.zeros((0, 2)), np.zeros(0, int)
        else:
            cam, p = camera(name)
            _POINTS[name] = kolb_point_set(cam.info(), p["sensorWidth"], p["focalDistance"])
            cam.close()
    return _POINTS[name]


def strided(a, most):
    """every k-th row of a, k fixed by its length: at most `most` rows"""
    return a[:: max(1, -(-len(a) // most))]


_RAYS = {}


def ray_set(oracle_lib, cam, name):
    """(records (m,8) f32, number of leading live forward records): a stride of the lens's live forward records, then the rejection
    families made from a stride of them, random lines and the non-finite rays; m <= MAX_RAYS.  Cached and not to be written to"""
    if name not in _RAYS:
        info = cam.info()
        _, o, d, w = oracle_records(oracle_lib, name)
        o, d = o[w > 0], d[w > 0]
        lo, ld = strided(o, 3072), strided(d, 3072)
        fo, fd = strided(o, 512), strided(d, 512)
        sets = [(lo, ld)] + list(tc.rejection_families(info, fo, fd).values()) + [tc.random_lines(info, 1024), tc.non_finite_rays()]
        rays = np.ascontiguousarray(np.concatenate([records(a, b) for a, b in sets]), F32)
        assert len(rays) <= MAX_RAYS
        rays.setflags(write=False)
        _RAYS[name] = rays, len(lo)
    return _RAYS[name]

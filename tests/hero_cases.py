"""What the hero-wavelength tests share besides the reference (tests/hero_ref.py, re-exported here): the cameras (CAMERAS), their
inputs (inputs()), the cached reference of each (reference()), the census of the families a batch exercises (census()) and the table
it is pinned in (CENSUS).  A plain helper module, imported by tests/test_hero_cpu.py and tests/test_hero_reference_gpu.py."""
from collections import OrderedDict

import numpy as np

from zoic_amd import PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states

import machine_lens_corpus as mlc
from fuzz_cameras import EXAMPLE_CAMERA, EXAMPLE_LENSES, LAMBDA_EDGES, perturbed_prescription
from hero_ref import LOST, REJECTED, Indices, hero_reference, oracle_camera, same_words, valid, words_of  # noqa: F401 (re-exported)
from spectral_ref import LAMBDA_D, WAVES as SPECTRAL_WAVES

N = 4096
OUT_OF_TRIES = 26          # the try count of a ray that ends without an accepted try (zoic.cpp:1951: tries > 25)
# fuzz_cameras.WAVES (tests/test_hero_reference_gpu.py holds the two equal): both ends of the range, their in-range
# neighbours, the F, d and C lines
WAVES = np.array([360.0, LAMBDA_EDGES[1], 405.0, 486.1327, LAMBDA_D, 656.2725, 760.0, LAMBDA_EDGES[3], 830.0], np.float32)


# ---- the cameras ---------------------------------------------------------------------------------------------------------------
class Spec:
    """one camera of the hero tests: update() parameters, prescription text and V-numbers (file order) where it is given them"""

    def __init__(self, params, lens=None, abbe=None):
        self.params, self.lens, self.abbe, self._dispersion = params, lens, abbe, None

    @property
    def text(self):
        return None if self.lens is None else self.lens.text

    def camera(self, device=0, precision=PRECISION_STRICT):
        cam = ZoicCamera(device=device)
        if self.lens is not None:
            self.lens.load(cam)
        elif self.abbe is not None:
            cam.set_abbe_numbers(self.abbe)
        p = self.params
        if p.get("useImage"):
            if device < 0:
                p = dict(p, useImage=False)          # a tables-only camera: the dispersion table does not depend on the image
            else:
                cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(precision)
        cam.update(**p)
        return cam

    def dispersion(self):
        if self._dispersion is None:
            cam = self.camera(device=-1)
            self._dispersion = cam.dispersion()
            cam.close()
        return self._dispersion


def _shipped(cfg, abbe=None, **over):
    p = camera_params(cfg)
    p.update(over)
    if abbe is not None:   # DOUBLE_GAUSS ships no V-numbers
        cam = ZoicCamera(device=-1).update(**dict(p, useImage=False))
        count = cam.info()["lensCount"]
        cam.close()
        abbe = np.full(count, abbe, np.float32)
    return Spec(p, abbe=abbe)


def _make_cameras():
    c = OrderedDict()
    c["C2"] = lambda: _shipped("C2")
    c["C5"] = lambda: _shipped("C5")
    c["C2-nolut"] = lambda: _shipped("C2", kolbSamplingLUT=False)
    c["C5-exposure+"] = lambda: _shipped("C5", exposureControl=1.5)
    c["C5-exposure-"] = lambda: _shipped("C5", exposureControl=-0.75)
    c["C3-bokeh-V50"] = lambda: _shipped("C3", abbe=50.0)
    for name in mlc.NAMES:
        c[name] = (lambda name=name: Spec(mlc.params(name), lens=mlc.LENSES[name]))
    # the two cameras of the spectral hostile fuzz's explicit examples (fuzz_cameras.EXAMPLE_LENSES behind EXAMPLE_CAMERA)
    for i, args in enumerate(EXAMPLE_LENSES):
        p = {key: v for key, v in EXAMPLE_CAMERA.items() if key != "image"}
        p.update(sensorHeight=p["sensorWidth"] / 1.5, useImage=False, lensDataPath="mem:hero_example_%d" % i)
        c["example-%d" % i] = (lambda p=p, args=args: Spec(p, lens=perturbed_prescription(*args, abbe=True)))
    return c


_MAKERS = _make_cameras()
CAMERAS = [name for name in _MAKERS if not name.startswith("example-")]      # what the issue lists: 6 shipped + the 10 corpus lenses
HOSTILE_CAMERAS = ["example-0", "example-1", "mori-6", "rear-9", "petzval-5"]
SHAPES_CAMERAS = ["C5"] + list(mlc.LARGE_BATCH)                              # k = 2, 4 and 8
FAST_CAMERAS = ["C5"] + list(mlc.ACCURACY)
_SPECS = {}


def spec(name):
    if name not in _SPECS:
        _SPECS[name] = _MAKERS[name]()
    return _SPECS[name]


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
WIDE_EVERY, WIDE_SCALE = 16, 3.0


def samples(n, seed=11):
    """(n, 4) float32: screen samples over the sensor (aspect 1.5), lens samples over the unit square; every WIDE_EVERY-th row's
    screen sample is stretched by WIDE_SCALE, past the sensor's edge and, far enough out, past the exit-pupil LUT's last key (the
    LUT-miss and dead-pixel endings)"""
    rs = np.random.RandomState(seed)
    s = np.stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n) / 1.5, rs.uniform(0, 1, n), rs.uniform(0, 1, n)], 1)
    s[WIDE_EVERY // 2::WIDE_EVERY, :2] *= WIDE_SCALE
    return np.ascontiguousarray(s, np.float32)


def palette(n, k, seed=3):
    """(n, k) float32 wavelengths drawn from WAVES per (row, column): neighbouring lanes trace at different wavelengths, and the oracle
    still runs one group per wavelength"""
    return WAVES[np.random.RandomState(seed).randint(len(WAVES), size=(n, k))].astype(np.float32)


# Rows that fill a camera's thin families.  The first N rows of inputs() give some cameras fewer than FAMILY_MIN lost companions,
# companions of retried heroes or left-out companions (census()).  For those cameras the last len(EXTRA[name]) of the first N rows are
# replaced by the rows of a second, larger batch -- samples(POOL, seed + 90), palette(POOL, k, seed + 91), ray_rng_states(POOL, seed +
# 92) -- at these indices: rows in which the reference alone (the oracle, k = 4, seed 11) finds one of the thin families, taken in
# index order until each reaches 24.  mori-4 has no left-out companion among all 262 144 rows of that batch (THIN).
POOL = 1 << 18
EXTRA = {
    "C2": [29, 102, 187, 348, 539, 3891, 4464, 5796, 5938, 7461, 8775, 10042, 10052, 10304, 10518, 11927, 11940, 12273, 12756, 13380],
    "C2-nolut": [1775, 2525, 2988, 3145, 3154, 3545, 4033, 5240, 5466, 6058, 7349, 8517, 12002, 13812, 15777, 16822, 18998, 19094, 19902, 22573,
                 24054, 24454, 28672, 29093, 29766, 31217, 38263],
    "tessar-5": [102, 617, 1335, 1723, 2214, 2865, 2896, 5564, 5796, 8267, 10093, 12419, 13324, 13562, 14320],
    "triplet-4": [29, 102, 10015, 12756, 24828, 33428, 36385, 38853, 54383, 55694, 56491, 60732, 69698, 92411, 102684, 122016, 125265],
    "mori-6": [140, 6069, 6324, 6502, 7876, 11940, 17643, 24828, 26880, 33741, 36287, 38505, 40638, 41319, 42160, 46986, 48188],
    "mori-4": [813, 2187, 2292, 4132, 7461, 7950, 8953, 10578, 11215, 13623, 14527, 15125, 16126, 16409, 21151, 23181, 23482, 25159, 25990, 28001,
               31496],
}


def inputs(n=N, k=4, seed=11, name=None):
    """(samples, wavelengths, rng states) of the standard batch of camera `name` (None: no camera's extra rows)"""
    s, lam, st = samples(n, seed), palette(n, k, seed + 1), ray_rng_states(n, seed=seed + 2)
    rows = EXTRA.get(name)
    if rows and n >= N:
        at = slice(N - len(rows), N)
        s[at], lam[at], st[at] = samples(POOL, seed + 90)[rows], palette(POOL, k, seed + 91)[rows], ray_rng_states(POOL, seed=seed + 92)[rows]
    return s, lam, st


_REFERENCE = {}


def reference(oracle_lib, name, n=N, k=4, seed=11):
    """hero_reference of camera `name` on inputs(n, k, seed, name), computed once: (samples, lam, states, words, counters, details); not
    to be written to"""
    key = (name, n, k, seed)
    if key not in _REFERENCE:
        sp = spec(name)
        s, lam, st = inputs(n, k, seed, name)
        words, counters, det = hero_reference(oracle_lib, sp.params, sp.dispersion(), s, lam, st, lens_text=sp.text, details=True)
        for a in (s, lam, st, words, det["starts"], det["planes"], det["flags"]):
            a.setflags(write=False)
        _REFERENCE[key] = s, lam, st, words, counters, det
    return _REFERENCE[key]


# the two cameras of the device tests of the lens losses (tests/test_transmittance_gpu.py, tests/test_ghost_gpu.py) and their reference
LOSS_CAMERAS = {"C2": "C2", "C3": "C3-bokeh-V50"}     # C3 ships no V-numbers: V = 50 on every glass, so that the wavelength matters
_LOSS_REFERENCE = {}


def cycled(n, k):
    """(n, k) wavelengths cycled from spectral_ref.WAVES, every row starting one further on: rows and columns both differ"""
    return SPECTRAL_WAVES[(np.arange(n)[:, None] * (k + 1) + np.arange(k)[None, :]) % len(SPECTRAL_WAVES)].astype(np.float32)


def loss_reference(oracle_lib, name, k, lam=None, key=None):
    """samples, wavelengths, states and the hero reference (words, starts) of N rows: computed once, never written to"""
    key = (name, k, key)
    if key not in _LOSS_REFERENCE:
        sp = spec(name)
        s, _, st = inputs(N, k, 11, name)
        lam = cycled(N, k) if lam is None else lam
        words, _, det = hero_reference(oracle_lib, sp.params, sp.dispersion(), s, lam, st, lens_text=sp.text, details=True)
        for a in (s, lam, st, words, det["starts"]):
            a.setflags(write=False)
        _LOSS_REFERENCE[key] = s, lam, st, words, det["starts"]
    return _LOSS_REFERENCE[key]


def oracle_columns(oracle_lib, sp, s, lam, st):
    """the oracle's own ray at every (row, column)'s wavelength (fuzz_cameras._oracle_spectral on the n k pairs, each with its row's
    sample and stream): planes (7, n, k) float32, flags (n, k); what the consistency check and the census hold the reference against"""
    from fuzz_cameras import _oracle_spectral
    n, k = lam.shape
    r = _oracle_spectral(oracle_lib, sp.params, sp.dispersion(), np.repeat(s, k, 0), np.ascontiguousarray(lam).reshape(n * k), np.repeat(st, k, 0),
                         lens_text=sp.text)[0]
    return r["planes"].reshape(7, n, k), r["flags"].astype(np.uint32).reshape(n, k)


def trace_starts(oracle_lib, sp, starts, lam):
    """the starts (n, 6), each once through the lens at its own wavelength lam (n,): ok (n,) bool, ends (n, 6) float32"""
    oc = oracle_camera(oracle_lib, sp.params, sp.text, None)
    idx = Indices(oc, sp.dispersion())
    ok, ends = np.zeros(len(lam), bool), np.zeros((len(lam), 6), np.float32)
    for w in np.unique(lam):
        rows = np.nonzero(lam == w)[0]
        idx.at(w)
        ok[rows], ends[rows] = oc.trace_rays(starts[rows])
        idx.restore()
    oc.close()
    return ok, ends


# ---- the census ----------------------------------------------------------------------------------------------------------------


def census(words, own_tries=None):
    """what a batch exercises, from the reference's words alone (valid wavelengths throughout):
      live          heroes of weight != 0
      through       companions that come through
      lost          companions of live heroes that are lost
      of_retried    companions (through or lost) of live heroes with an accepted try > 0
      left_out      own_tries given (the oracle's own try counts per (row, column)): companions of live heroes that the oracle accepts
                    at an EARLIER try than the hero's -- the rows the inference of test_companions_against_the_oracle knew nothing about
      out_of_tries  heroes of weight 0: 26 tries.  Dead pixels, retry-dead rays and rays whose 27 tries all failed end here alike
      lut_miss      heroes with flag bit 6 (outside the exit-pupil LUT)
      dead_in_lut_miss  heroes with bit 6 and weight 0: outside the LUT every try shoots the same direction, a dead pixel (setup_ray).
                    The flags tell no more: a retry-dead ray inside the LUT ends like any ray out of tries."""
    f = words[:, :, 7]
    w = words[:, :, 6].view(np.float32)
    hero_tries = (f[:, 0] >> 1) & 31
    live = w[:, 0] != 0
    comp_lost = (f[:, 1:] & LOST) != 0
    c = dict(live=int(live.sum()), through=int((~comp_lost[live]).sum()), lost=int(comp_lost[live].sum()),
             of_retried=int((live & (hero_tries > 0)).sum()) * (f.shape[1] - 1),
             out_of_tries=int((~live & (hero_tries == OUT_OF_TRIES)).sum()), lut_miss=int(((f[:, 0] >> 6) & 1).sum()),
             dead_in_lut_miss=int((~live & (((f[:, 0] >> 6) & 1) == 1)).sum()))
    assert ((hero_tries == OUT_OF_TRIES) | live).all()
    if own_tries is not None:
        c["left_out"] = int((live[:, None] & (own_tries[:, 1:] < hero_tries[:, None])).sum())
    return c


# The census of reference(name) for every camera of CAMERAS (n = 4096, k = 4, the camera's standard inputs), computed from the reference alone by
# tests/test_hero_cpu.py::test_consistency_with_the_oracle_and_census, which holds every entry exactly: a change of the inputs, of
# the oracle or of the reference shows here first.  The GPU tests (tests/test_hero_reference_gpu.py) find the same counts in the
# library's output.  Every family has at least FAMILY_MIN rows except the
# (camera, family) pairs of THIN: families the camera cannot produce, each with the reason.
FAMILY_MIN = 16
_COLUMNS = ["live", "through", "lost", "of_retried", "left_out", "out_of_tries", "lut_miss", "dead_in_lut_miss"]
_ROWS = """
C2             3061   9158    25   567   25  1035   99   99
C5              670   1965    45   714   50  3426  100  100
C2-nolut       2208   6599    25  6282   25  1888    0    0
C5-exposure+    670   1965    45   714   50  3426  100  100
C5-exposure-    670   1965    45   714   50  3426  100  100
C3-bokeh-V50   3901  11670    33  2121   46   195  100  100
triplet-4      2287   6837    24   105   25  1809   61   61
fisheye-5      3977  11823   108  1095   99   119   62   62
mori-6         2945   8811    24   114   24  1151   61   61
double-3       3930  11594   196  1653  177   166   62   62
tessar-5       1944   5808    24   603   24  2152   61   61
petzval-2      1339   3993    24  1146   16  2757   62   62
mori-4         1515   4520    25    24    0  2581   61   61
rear-9         1915   4877   868  3894  423  2181   62   62
rear-12        3439   9522   795  6078  533   657   62   62
petzval-5       910   2625   105   984   67  3186   62   62
"""
CENSUS = {r.split()[0]: dict(zip(_COLUMNS, map(int, r.split()[1:]))) for r in _ROWS.strip().splitlines()}
_NO_LUT = "kolbSamplingLUT is off: there is no exit-pupil LUT to miss"
_NONE_FOUND = ("the stop is the first interface and about one live hero in 1500 retries: among the 262 144 rows of the second batch (EXTRA) the oracle "
               "accepts no companion of a retried hero at an earlier try")
THIN = {("C2-nolut", "lut_miss"): _NO_LUT, ("C2-nolut", "dead_in_lut_miss"): _NO_LUT, ("mori-4", "left_out"): _NONE_FOUND}

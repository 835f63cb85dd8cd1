"""A CPU reference of the whole hero-wavelength call (zoic_create_rays_hero_device, zoic_amd/csrc/hero.hpp), shared by
tests/test_hero_cpu.py, tests/test_hero_gpu.py and tests/test_hero_reference_gpu.py: a plain helper module.

hero_reference() builds all n x k records and the counter deltas from the oracle alone:
  * column 0 is the oracle's ray at the hero's wavelength, the lens table's indices swapped per wavelength as
    fuzz_cameras._oracle_spectral does it, through OracleCamera.create_rays_starts, which also hands back the (origin, dir) the ray's
    last try began with -- the accepted try's start where the weight is not 0.  With the exit-pupil LUT on a retry translates both
    components of its lens point (zoic.cpp:1933), the first try only x (zoic.cpp:1914): the start cannot be rebuilt from a
    substituted sample, it has to be recorded;
  * a companion is that start through OracleCamera.trace_rays with the indices of its own wavelength: it comes through -> the traced
    (o, d) x -1, the hero's weight and flags; it does not -> zeros and the hero's flags | RAY_COMPANION_LOST;
  * a hero of weight 0 has lost companions; an invalid companion wavelength is a rejected record (0x80, zeros); an invalid hero
    rejects the row, which then counts nowhere; the counters are those of column 0.
Not modelled: the retry-dead ray one of whose draws lands on the disk's centre (2e-15 per draw; a NaN ray of weight != 0 whose
companions the library declares lost).  hero_reference asserts that its inputs hold none.

The cameras, inputs and census the hero tests share are in tests/hero_cases.py."""
import numpy as np

from zoic_amd import RAY_COMPANION_LOST, RAYTRACED
from zoic_amd.workloads import hexagon_bokeh

from device_cases import bits_f32 as _bits
from spectral_ref import spectral_iors

LOST = RAY_COMPANION_LOST
REJECTED = 0x80


def valid(lam):
    """spectral.hpp spectral_valid: 360 <= lambda <= 830 (NaN is not)"""
    lam = np.asarray(lam, np.float32)
    with np.errstate(invalid="ignore"):
        return (lam >= np.float32(360.0)) & (lam <= np.float32(830.0))


def oracle_camera(oracle_lib, params, lens_text, image):
    oc = oracle_lib.OracleCamera()
    if lens_text is not None:
        oc.set_lens_text(lens_text)
    if params.get("useImage"):
        oc.set_bokeh_image(hexagon_bokeh() if image is None else image)
    oc.update(**params)
    return oc


class Indices:
    """the oracle camera's lens table with the indices of one wavelength written in, the d-line's back on exit"""

    def __init__(self, oc, dispersion):
        self.count = 0
        if dispersion is None:        # a lens model that ignores the wavelength
            return
        self.count = oc._L.zo_lens_count(oc._h)
        self.le = oc._L.zo_lenses(oc._h)
        self.nd = np.array([self.le[i].ior for i in range(self.count)], np.float32)
        assert np.array_equal(self.nd, dispersion["ior_d"])
        self.b = dispersion["cauchy_b"]

    def at(self, lam):
        ior = spectral_iors(self.nd, self.b, lam) if self.count else None
        for i in range(self.count):
            self.le[i].ior = float(ior[i])

    def restore(self):
        for i in range(self.count):
            self.le[i].ior = float(self.nd[i])


def hero_reference(oracle_lib, params, dispersion, samples, lam, states, lens_text=None, image=None, details=False, oc=None):
    """(words, counters): words (n, k, 8) uint32, all 8 words of every record of the call; counters: the deltas of succesRays,
    vignettedRays and totalInternalReflection.  details=True adds a dict: starts (n, 6) float32 and hero (planes (7, n), flags (n,)),
    rows of an invalid hero zero.
    oc: an updated oracle camera the caller owns (its history is the camera's: tests/update_sequences.py) instead of a fresh one behind
    params, lens_text and image; it is not closed, and its lens table holds the d-line indices again on return."""
    s = np.ascontiguousarray(samples, np.float32)
    lam = np.ascontiguousarray(lam, np.float32)
    st = np.ascontiguousarray(states, np.uint32)
    n, k = lam.shape
    assert s.shape == (n, 4) and st.shape == (n, 4)
    ok_lam = valid(lam)
    own = oc is None
    if own:
        oc = oracle_camera(oracle_lib, params, lens_text, image)
    thin = params.get("lensModel", RAYTRACED) != RAYTRACED
    idx = Indices(oc, None if thin else dispersion)
    planes = np.zeros((7, n), np.float32)
    flags = np.zeros(n, np.uint32)
    starts = np.zeros((n, 6), np.float32)
    # ---- column 0: the oracle at the hero's wavelength, start recorded -----------------------------------------------------
    before = oc.counters()
    hero_rows = np.nonzero(ok_lam[:, 0])[0]
    for w in np.unique(lam[hero_rows, 0]):
        rows = hero_rows[lam[hero_rows, 0] == w]
        idx.at(w)
        r = oc.create_rays_starts(s[rows], st[rows])
        idx.restore()
        planes[:, rows] = r["planes"]
        flags[rows] = r["flags"]
        starts[rows] = r["starts"]
    after = oc.counters()
    counters = {key: after[key] - before[key] for key in after}
    live = ok_lam[:, 0] & (planes[6] != 0)
    # the one case that is not modelled must not be among the inputs: a retried hero of weight != 0 whose origin is NaN though its
    # screen sample is finite (kolb_pool_body.hpp dead_ray_end: a retry's draw at the centre of the disk)
    nan_draw = live & ((flags & 1) != 0) & np.isnan(planes[0:3]).all(0) & np.isfinite(s[:, :2]).all(1)
    assert not nan_draw.any(), ("a retry's NaN draw is outside this reference", np.nonzero(nan_draw)[0][:4])
    words = np.zeros((n, k, 8), np.uint32)
    words[:, 0, :7] = _bits(planes).T
    words[:, 0, 7] = flags
    words[~ok_lam[:, 0], :, 7] = REJECTED
    if thin:
        # the other lens models ignore the wavelength (hero.hpp launch_hero_replicate): the record in every valid column of a valid row
        for j in range(1, k):
            words[:, j] = np.where((ok_lam[:, 0] & ok_lam[:, j])[:, None], words[:, 0], words[:, j])
            words[ok_lam[:, 0] & ~ok_lam[:, j], j, 7] = REJECTED
        k = 1
    # ---- companions: the hero's start once through the indices of their own wavelength ------------------------------------------
    for j in range(1, k):
        col = ok_lam[:, 0] & ok_lam[:, j]
        words[ok_lam[:, 0] & ~ok_lam[:, j], j, 7] = REJECTED
        words[col, j, 7] = flags[col] | LOST                       # lost until it comes through
        traced = np.nonzero(col & live)[0]
        for w in np.unique(lam[traced, j]):
            rows = traced[lam[traced, j] == w]
            idx.at(w)
            ok, ends = oc.trace_rays(starts[rows])
            idx.restore()
            through = rows[ok]
            words[through, j, :6] = _bits(ends[ok] * np.float32(-1.0))        # zoic.cpp:1960-1961
            words[through, j, 6] = _bits(planes[6, through])
            words[through, j, 7] = flags[through]
    if own:
        oc.close()
    if details:
        return words, counters, dict(starts=starts, planes=planes, flags=flags)
    return words, counters


def same_words(a, b):
    """(n, k) bool: all 8 words of the record identical, a NaN equal to any NaN in the seven float words"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    fa, fb = a[..., :7].view(np.float32), b[..., :7].view(np.float32)
    same = (a == b)
    same[..., :7] |= np.isnan(fa) & np.isnan(fb)
    return same.all(-1)


def words_of(result):
    """(n, k, 8) uint32 of a numpy create_rays_hero result"""
    r = result["rays"]
    return np.ascontiguousarray(r).view(np.uint32).reshape(r.shape + (8,))

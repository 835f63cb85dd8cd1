"""Cameras, scene points, wavelengths, aims' numbers and cached restatements for pupil bounds and lens splats on the pinned corpus of
machine-made lenses (machine_lens_corpus.py), shared by tests/test_pupil_splat_corpus_cpu.py and tests/test_pupil_splat_corpus_gpu.py.

The corpus parameters carry no useDof, which the host drivers index: every camera here is updated with dict(params, useDof=True) (a
RAYTRACED camera ignores the value).

Points of a lens (points(name): at most 64 and seven specials, cached, read only), with their depth index (SPECIAL = -1 for a special)
and their kind (CHIEF, MOVED, SPECIAL_KIND):
  chief     mc.strided(mc.point_set(name)[0], 48): points on chief rays at the four depths of reverse_ref.kolb_point_set (0: 1e-3 cm
            in front of the front element, 1: focalDistance, 2: ten times that, 3: 1e4 cm);
  moved     16 of those at depths 1 to 3 (a stride of them), moved across the axis off their chief ray by 0.3 R (every other one) and
            0.9 R (the rest), R from cam.pupil_square(): 48 + 16 = 64;
  specials  on the axis at 20 and at 1e4 cm; pz equal to the aims' plane z (dir.z = 0: kTbAway); behind the lens; a NaN point; far
            along the direction of the last chief-ray point at 1e15 and 1e25 cm (r2 r and r2 overflow in the splat's angle).
petzval-5 (mc.OUTSIDE), whose point set is empty, has the specials only; its far points lie along a fixed direction.

The SINGLE_LANE and FULL_WAVE rows of a lens and lattice (rows_of_interest) are taken from the restatement's passing mask: a point
whose passing aims all have the same a & 63 (one lane of the wave holds the whole pupil; the aims of lane l are a = l, l + 64, ...),
and a point with count >= 64.  Which lenses have none of the first kind at which lattice is measured in
tests/test_pupil_splat_corpus_cpu.py::test_sparse_and_full_pupils_are_present; fisheye-5 has one at every lattice and stands in.
device_order puts those rows first in the batch the device tests send, and f64_rows names the two points (1e15 and 1e25 cm) that the f64
comparison leaves out.  A helper, not a test."""
import functools

import numpy as np

import backward_spectral_ref as bs
import host_drivers
import machine_lens_corpus as mc
import pupil_cases as pc
import pupil_driver
import pupil_ref
import splat_driver
import splat_ref
import traceback_jacobian_ref as jr

F32 = np.float32
LATTICES = pc.LATTICES
WINDOW = pc.WINDOW
AIMS = (1, 5, 64)
SPLAT_LATTICE = 16           # the lattice of the bounds the splats are drawn in
SPECIAL = -1                 # the depth index of a special point
N_SPECIAL = 7
CHIEF, MOVED, SPECIAL_KIND = 0, 1, 2   # the kinds of points
STAND_IN = "fisheye-5"       # the lens whose set has a single-lane point at every lattice
IN_DOMAIN = [n for n in mc.NAMES if n != mc.OUTSIDE]


class Lens:
    """one corpus lens: its tables-only camera, the parameters the host drivers take, the f64 trace, the aims' plane and square"""

    def __init__(self, name):
        self.name = name
        self.cam, p = mc.camera(name)
        self.p = dict(p, useDof=True)
        self.info, self.disp = self.cam.info(), self.cam.dispersion()
        self.T = bs.SpectralTraceBack(self.info, self.p, self.disp)
        self.z, self.R = pupil_ref.square(self.info, self.p)
        z, R = self.cam.pupil_square()
        assert (F32(z), F32(R)) == (self.z, self.R)
        self.s = jr.scales(self.info, self.p)


@functools.lru_cache(maxsize=None)
def lens(name):
    return Lens(name)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def points(name):
    """(points (n,3) float32, depth index (n,), samples (n,2): the known sample of a chief-ray point, NaN elsewhere, kind (n,)),
    read only"""
    L = lens(name)
    z, R = float(L.z), float(L.R)
    P, S, D = mc.point_set(name)
    rows, depth, smp, kind = [], [], [], []
    along = _unit([0.3, -0.2, -1.0])
    if len(P):
        idx = mc.strided(np.arange(len(P)), 48)
        rows += [P[i].astype(np.float64) for i in idx]
        depth += [int(D[i]) for i in idx]
        smp += [S[i] for i in idx]
        kind += [CHIEF] * len(idx)
        deep = mc.strided(np.array([i for i in idx if D[i] >= 1]), 16)
        for k, i in enumerate(deep):
            q = P[i].astype(np.float64)
            off = (0.3 if k % 2 == 0 else 0.9) * R
            q[0] -= off * (1.0 if q[0] >= 0 else -1.0)      # across the axis
            q[1] += 0.5 * off * (1.0 if k % 4 < 2 else -1.0)
            rows.append(q)
            depth.append(int(D[i]))
            smp.append((np.nan, np.nan))
            kind.append(MOVED)
        along = _unit(P[idx[-1]])
    special = [(0.0, 0.0, -20.0), (0.0, 0.0, -1.0e4), (0.1 * R, -0.05 * R, z), (0.05, 0.0, 5.0), (np.nan, 0.0, -100.0),
               tuple(1.0e15 * along), tuple(1.0e25 * along)]
    assert len(special) == N_SPECIAL
    rows += [np.array(q, np.float64) for q in special]
    depth += [SPECIAL] * N_SPECIAL
    smp += [(np.nan, np.nan)] * N_SPECIAL
    kind += [SPECIAL_KIND] * N_SPECIAL
    pts = np.ascontiguousarray(np.array(rows), F32)
    assert len(pts) <= 64 + N_SPECIAL
    out = pts, np.array(depth), np.array(smp, np.float64), np.array(kind)
    for a in out:
        a.setflags(write=False)
    return out


# the specials' rows, from the end
AXIS_NEAR, AXIS_FAR, ON_PLANE, BEHIND, NON_FINITE, FAR_15, FAR_25 = range(-N_SPECIAL, 0)


def wavelengths(n):
    """bs.mixed_wavelengths: valid and rejected wavelengths interleaved, every fourth point rejected"""
    lam = bs.mixed_wavelengths(n)
    lam.setflags(write=False)
    return lam


def u(n, m, seed=0):
    """(n, m, 2) float32, seeded, with the specials of test_splats_gpu._u: the box's centre, a corner, a NaN, a value outside the
    unit square"""
    a = np.random.default_rng(1000 * n + m + seed).random((n, m, 2)).astype(F32)
    a[0, 0] = (0.5, 0.5)
    a[0, m - 1] = (0.0, F32(1.0) - F32(2.0 ** -24)) if m > 1 else a[0, 0]
    if m > 2:
        a[n // 2, 1] = (np.nan, 0.5)
        a[n - 1, 2] = (-1.0, 2.0)
    return a


@functools.lru_cache(maxsize=None)
def reference(name, G, windowed=False, spectral=False):
    """(records, passing mask (n, G^2)) of the restatement pupil_ref.reference on points(name), cached and read only"""
    L = lens(name)
    pts = points(name)[0]
    lam = wavelengths(len(pts)) if spectral else None
    ref, ok = pupil_ref.reference(host_drivers.traceback(), L.cam, L.p, pts, G, WINDOW if windowed else None, lam)
    ref.setflags(write=False)
    ok.setflags(write=False)
    return ref, ok


def host_bounds(name, G, windowed=False, spectral=False, pts=None, lam=None, wave_lane=None):
    """the host twin's records (csrc/pupil_bounds.hpp compiled for the host) of points(name), or of pts (with lam); wave_lane: by the
    kernel's walk of 64 lanes and its butterfly of pupil_merge, the record lane wave_lane holds (pupil_driver.py)"""
    L = lens(name)
    if pts is None:
        pts = points(name)[0]
        lam = wavelengths(len(pts)) if spectral else None
    return pupil_driver.drive_pupil(pupil_driver.pupil(), L.cam, L.p, pts, G, WINDOW if windowed else None, lam,
                                    None if lam is None else L.disp, wave_lane)


def host_splats(name, pts, bounds, uu, lam=None):
    """the host twin's records (csrc/splat.hpp compiled for the host)"""
    L = lens(name)
    return splat_driver.drive_splat(splat_driver.splat(), L.cam, L.p, pts, bounds, uu, lam, None if lam is None else L.disp)


@functools.lru_cache(maxsize=None)
def splat_reference(name, m, spectral=False):
    """(records (n, m), dirs (n m, 3), J (n m, 12)) of the restatement splat_ref.reference on points(name), in the boxes of the
    restatement's own bounds at SPLAT_LATTICE (d-line bounds for the d-line form, spectral bounds for the spectral one); read only"""
    L = lens(name)
    pts = points(name)[0]
    b = reference(name, SPLAT_LATTICE, False, spectral)[0]
    out = splat_ref.reference(L.cam, pts, b, u(len(pts), m), wavelengths(len(pts)) if spectral else None)
    for a in out:
        a.setflags(write=False)
    return out


def rows_of_interest(ok):
    """(single-lane rows, full-wave rows) of a passing mask (n, G^2): all passing aims in one lane a & 63; count >= 64"""
    lane = np.arange(ok.shape[1]) & 63
    single = [i for i in range(len(ok)) if ok[i].any() and len(set(lane[ok[i]].tolist())) == 1]
    return np.array(single, int), np.flatnonzero(ok.sum(1) >= 64)


def device_order(name, G):
    """the order the device tests give the points of a lens at lattice G, so that the prefixes n = 1, 3, 4, 5 hold the rows that
    matter and not five empty boxes: a single-lane row (if the lens has one), the two sparsest non-empty rows, two full-wave rows (if
    any), then every other row in its own order.  (n,) indices, each row once."""
    ref, ok = reference(name, G)
    single, full = rows_of_interest(ok)
    some = np.flatnonzero(ref["count"] > 0)
    sparse = some[np.argsort(ref["count"][some], kind="stable")][:2]
    first = []
    for i in list(single[:1]) + list(sparse) + list(full[:2]):
        if int(i) not in first:
            first.append(int(i))
    return np.array(first + [i for i in range(len(ref)) if i not in first], int)


def f64_trace(L, o, d, lam=None):
    """the f64 trace-back (TraceBack.trace; lam: SpectralTraceBack.trace_at) of the f32 rays (o, d)"""
    return L.T.trace(o, d) if lam is None else L.T.trace_at(o, d, lam)


def f64_rows(name):
    """(n,) bool: the points whose rays the f64 trace is compared on -- all but the two at 1e15 and 1e25 cm.  From there neither trace
    says anything about the line: the library moves the start point to the front vertex plane with one fmaf per coordinate, exact to
    an ulp of the start point's own size (6e7 cm at 1e15 cm), TraceBack.trace cancels |L|^2 - tca^2 completely in f64, and dir =
    P - A no longer holds the aim.  Their records are held bit for bit to the restatement and to the device."""
    use = np.ones(len(points(name)[0]), bool)
    use[[FAR_15, FAR_25]] = False
    return use

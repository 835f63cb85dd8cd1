"""An independent restatement of the pupil bounds (zoic_amd/csrc/pupil_bounds.hpp), written from the definition: the n G^2 rays are
built in numpy f32 with the definition's three operations (an int -> f32 conversion, a multiplication by R / G, a subtraction from P),
traced back by code that is already pinned -- the host driver of csrc/traceback.hpp (host_drivers.drive_traceback, held against f64
by tests/test_traceback_cpu.py) or, at a wavelength, the library's zoic_trace_back_ray_spectral -- and reduced with numpy.
A helper, not a test."""
import numpy as np

import traceback_cases as tc
from host_drivers import drive_traceback
from zoic_amd import _capi

F32 = np.float32
DTYPE = np.dtype(_capi.PUPIL_BOUNDS_DTYPE)
OUTSIDE_WINDOW = 0            # the reason of an aim that traced back but landed outside the window
REASON_SHIFT = 16


def square(info, p):
    """(z of the aims' plane in the record frame, R): RAYTRACED the front vertex plane (the f32 running sum of the thicknesses, negated)
    and the root of the front row's housing2 (the largest f32 <= (aperture / 2)^2, at the stop also <= userApertureRadius^2); THINLENS
    z = 0 and the root of apertureRadius^2; any other camera (0, 0): it traces no ray"""
    if int(p["lensModel"]) == _capi.THINLENS:
        a = F32(info["apertureRadius"])
        return F32(0.0), np.sqrt(F32(a * a))
    n = int(info["lensCount"])
    if int(p["lensModel"]) != _capi.RAYTRACED or n == 0:
        return F32(0.0), F32(0.0)
    th = info["elements"][:n, 1].astype(F32)
    s = th[0]
    for t in th[1:]:
        s = F32(s + t)
    lim = (float(info["elements"][n - 1, 3]) * 0.5) ** 2
    h2 = F32(lim)
    if float(h2) > lim:
        h2 = np.nextafter(h2, F32(-np.inf))
    ua2 = F32(F32(info["userApertureRadius"]) * F32(info["userApertureRadius"]))
    if int(info["apertureElement"]) == n - 1 and ua2 < h2:
        h2 = ua2
    return F32(-s), np.sqrt(F32(h2))


def aims(G, R):
    """(ax, ay) of the G^2 aims in index order a = iy G + ix, each (G^2,) float32"""
    h = F32(R) / F32(G)
    c = (2 * np.arange(G) + 1 - G).astype(F32) * h
    return np.tile(c, G), np.repeat(c, G)


def rays(points, G, z, R):
    """origin, dir (n G^2, 3) float32: origin = P, dir = P - A, point-major"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 3)
    ax, ay = aims(G, R)
    A = np.stack([ax, ay, np.full(G * G, z, F32)], 1)
    o = np.repeat(pts, G * G, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (o.reshape(-1, G * G, 3) - A[None]).reshape(-1, 3).astype(F32)
    return o, d


def reduce(scr, fl, n, G, R, window=None):
    """the (n,) records of the traced rays (scr (n G^2, 2), fl (n G^2,)), and the (n, G^2) passing mask"""
    scr = scr.reshape(n, G * G, 2)
    fl = fl.reshape(n, G * G).astype(np.uint32)
    traced = (fl & 1) == 1
    inside = np.ones_like(traced)
    if window is not None:
        w = np.asarray(window, F32)
        with np.errstate(invalid="ignore"):
            inside = (scr[..., 0] >= w[0]) & (scr[..., 0] <= w[2]) & (scr[..., 1] >= w[1]) & (scr[..., 1] <= w[3])
    ok = traced & inside
    reason = np.where(traced, OUTSIDE_WINDOW, (fl >> 8) & 0xF).astype(np.uint32)
    ax, ay = aims(G, R)
    pitch = F32(2.0) * (F32(R) / F32(G))
    out = np.zeros(n, DTYPE)
    out["lattice"] = G * G
    for i in range(n):
        m = ok[i]
        bits = np.uint32(0)
        for r in np.unique(reason[i][~m]):
            bits |= np.uint32(1) << np.uint32(REASON_SHIFT + int(r))
        out["count"][i] = m.sum()
        if not m.any():
            out["flags"][i] = bits
            continue
        out["flags"][i] = bits | np.uint32(1)
        out["aim"][i] = [max(F32(ax[m].min() - pitch), F32(-R)), max(F32(ay[m].min() - pitch), F32(-R)),
                         min(F32(ax[m].max() + pitch), F32(R)), min(F32(ay[m].max() + pitch), F32(R))]
        out["screen"][i] = [scr[i, m, 0].min(), scr[i, m, 1].min(), scr[i, m, 0].max(), scr[i, m, 1].max()]
    return out, ok


def trace(driver, cam, p, o, d, lam=None):
    """(screen, flags) of rays: the pinned d-line host driver, or the library's host call at a wavelength per ray"""
    if lam is None:
        return drive_traceback(driver, cam, p, o, d)
    return tc.lib_trace(cam, o, d, lam)


def reference(driver, cam, p, points, G, window=None, lam=None):
    """the records of points (n,3) and the (n, G^2) mask of passing aims; lam: None (d-line) or (n,) wavelengths (nm), one per point"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 3)
    z, R = square(cam.info(), p)
    o, d = rays(pts, G, z, R)
    scr, fl = trace(driver, cam, p, o, d, None if lam is None else np.repeat(np.asarray(lam, F32), G * G))
    return reduce(scr, fl, len(pts), G, R, window)


def same_records(a, b):
    """bit for bit, every field (floats compared as their bits)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()

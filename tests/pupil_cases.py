"""Cameras and scene points shared by tests/test_pupil_bounds_cpu.py and tests/test_pupil_bounds_gpu.py.  A helper, not a test."""
import numpy as np

import traceback_cases as tc

F32 = np.float32
# name -> (traceback_cases configuration, parameter overrides); "C3-f8": the double Gauss stopped down to f/8
CAMERAS = {"C3": ("C3", {}), "C5": ("C5", {}), "triplet": ("triplet", {}), "C1": ("C1", {}), "C1-vignetting": ("C1-vignetting", {}),
           "C3-f8": ("C3", dict(fStop=8.0))}
RAYTRACED = ("C3", "C5", "triplet", "C3-f8")
LATTICES = (8, 16, 32)
# a film window that cuts the frame's right half and a strip at the bottom off
WINDOW = (-1.0, -0.25, 0.05, 0.6)
LAMBDAS = (450.0, 587.5618, 640.0)   # nm: the spectral cases cycle through these, plus one invalid wavelength
BAD_LAMBDA = 900.0


def params_of(name):
    cfg, over = CAMERAS[name]
    return dict(tc.params_of(cfg), **over)


def points(p):
    """(m,3) float32 scene points in the frame of the records (the scene at z < 0) for the camera parameters p, placed by the field
    (half of it: sensorWidth / 2 over focalLength): x = t field |z| lands near sx = -t.  On the axis and off it at 20, 100 and 1e4 cm,
    one at the field's edge, one behind the lens, one non-finite."""
    t = 0.5 * float(p["sensorWidth"]) / float(p["focalLength"])
    rows = [(0.0, 0.0, 100.0), (0.0, 0.0, 20.0), (0.0, 0.0, 1.0e4),
            (0.4, 0.2, 100.0), (-0.3, 0.15, 20.0), (0.5, -0.3, 1.0e4), (-0.7, 0.35, 100.0),
            (0.98, 0.0, 100.0)]                                           # the field's edge
    pts = [(a * t * z, b * t * z, -z) for a, b, z in rows]
    pts.append((0.05, 0.0, 5.0))                                          # behind the lens
    pts.append((np.nan, 0.0, -100.0))                                     # non-finite
    return np.array(pts, F32)


BEHIND, NON_FINITE = -2, -1   # rows of points()


def wavelengths(m):
    """(m,) float32: LAMBDAS in turn, the fourth point's invalid"""
    lam = np.array([LAMBDAS[i % len(LAMBDAS)] for i in range(m)], F32)
    lam[3] = F32(BAD_LAMBDA)
    return lam


def batch(p, n):
    """(n,3) float32: points() repeated with a small per-row shift, so that every row of a large batch is its own point"""
    base = points(p)
    reps = -(-n // len(base))
    k = np.arange(reps * len(base), dtype=np.float64) // len(base)
    pts = np.tile(base, (reps, 1)).astype(np.float64)
    pts[:, 0] += 0.013 * k
    pts[:, 1] -= 0.007 * k
    return np.ascontiguousarray(pts[:n], F32)

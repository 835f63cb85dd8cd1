"""Host build of csrc/pupil_bounds.hpp for the tests (through host_drivers._build: compiled once per process): the records of many
points in one call, at the d-line or at a wavelength per point.  A helper, not a test."""
import ctypes

import numpy as np

import host_drivers
from zoic_amd import _capi

PUPIL = r"""
#include "pupil_bounds.hpp"
// disp: count x (iorD, cauchyB), trace order, or NULL (d-line); lambda: one per point or NULL; window: 4 floats or NULL; out: n x 48 bytes
extern "C" int zpb_bounds(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior, const float *aperture,
                          int apertureElement, float userApertureRadius, float originShift, float sensorWidth, int useLUT, int lutSize, int domain,
                          float apertureRadius, float focalDistance, int useDof, float ovDistance, float ovRadius, const float *disp,
                          long n, const float *pts, const float *lambda, int G, const float *window, void *out)
{
    using namespace zoic;
    static_assert(sizeof(PupilBounds) == 48, "the record is 48 bytes");
    if (!pupil_lattice_valid(G)) return 1;
    TraceBackTable T;
    fill_traceback_table(T, model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius, originShift,
                         sensorWidth, useLUT != 0, lutSize, domain != 0, apertureRadius, focalDistance, useDof != 0, ovDistance, ovRadius);
    SpectralTable S{};
    S.count = count;
    for (int i = 0; disp && i < count && i < kMaxSurfaces; ++i) { S.iorD[i] = disp[2 * i]; S.cauchyB[i] = disp[2 * i + 1]; }
    BackwardDispersion D;
    fill_backward_dispersion(D, S);
    const PupilWindow W = window ? PupilWindow{window[0], window[1], window[2], window[3]} : PupilWindow{};
    PupilBounds *B = static_cast<PupilBounds *>(out);
    for (long i = 0; i < n; ++i)
        B[i] = lambda ? pupil_bounds_point_spectral(T, D, lambda[i], G, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], W)
                      : pupil_bounds_point(T, G, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], W);
    return 0;
}
"""


def pupil():
    """zpb_bounds, called through drive_pupil"""
    return host_drivers._build("pupil_bounds", PUPIL)


def drive_pupil(driver, cam, p, pts, G, window=None, lam=None, dispersion=None):
    """the records (n,) of _capi.PUPIL_BOUNDS_DTYPE the host build gives points (n,3); lam (n,) with dispersion = cam.dispersion()"""
    info = cam.info()
    n = info["lensCount"]
    el = [np.ascontiguousarray(info["elements"][:, k], dtype=np.float32) for k in range(4)]
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), _capi.PUPIL_BOUNDS_DTYPE)
    out["reserved"] = 0xDEAD
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    F = ctypes.c_float
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    lm = None if lam is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lam, np.float32), (len(pts),)))
    dp = None if dispersion is None else np.ascontiguousarray(np.stack([dispersion["ior_d"], dispersion["cauchy_b"]], 1), np.float32)
    assert (lm is None) == (dp is None) or p["lensModel"] != _capi.RAYTRACED
    rc = driver.zpb_bounds(int(p["lensModel"]), F(info["tan_fov"]), n, P(el[0]), P(el[1]), P(el[2]), P(el[3]), info["apertureElement"],
                           F(info["userApertureRadius"]), F(info["originShift"]), F(p["sensorWidth"]),
                           int(bool(p["kolbSamplingLUT"]) and len(info["lutKeys"]) > 0), len(info["lutKeys"]), int(not info["fastRunsStrict"]),
                           F(info["apertureRadius"]), F(p["focalDistance"]), int(bool(p["useDof"])), F(p.get("opticalVignettingDistance", 0.0)),
                           F(p.get("opticalVignettingRadius", 1.0)), P(dp), ctypes.c_long(len(pts)), P(pts), P(lm), int(G), P(w), P(out))
    assert rc == 0, rc
    return out

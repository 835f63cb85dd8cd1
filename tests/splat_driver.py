"""Host build of csrc/splat.hpp for the tests (through host_drivers._build: compiled once per process): the records of many points
and their m aims in one call, at the d-line or at a wavelength per point.  A helper, not a test."""
import ctypes

import numpy as np

import host_drivers
from zoic_amd import _capi

SPLAT = r"""
#include <cstring>
#include "splat.hpp"
// disp: count x (iorD, cauchyB), trace order, or NULL (d-line); lambda: one per point or NULL; bounds: n x 48 bytes; u: n x m x 2;
// out: n x m x 32 bytes
extern "C" int zsp_splats(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior, const float *aperture,
                          int apertureElement, float userApertureRadius, float originShift, float sensorWidth, int useLUT, int lutSize, int domain,
                          float apertureRadius, float focalDistance, int useDof, float ovDistance, float ovRadius, const float *disp,
                          long n, const float *pts, const void *bounds, const float *lambda, unsigned m, const float *u, void *out)
{
    using namespace zoic;
    static_assert(sizeof(Splat) == 32 && alignof(Splat) == 16, "the record is 32 bytes, 16-byte aligned");
    if (m == 0) return 1;
    TraceBackTable T;
    fill_traceback_table(T, model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius, originShift,
                         sensorWidth, useLUT != 0, lutSize, domain != 0, apertureRadius, focalDistance, useDof != 0, ovDistance, ovRadius);
    SpectralTable S{};
    S.count = count;
    for (int i = 0; disp && i < count && i < kMaxSurfaces; ++i) { S.iorD[i] = disp[2 * i]; S.cauchyB[i] = disp[2 * i + 1]; }
    BackwardDispersion D;
    fill_backward_dispersion(D, S);
    for (long p = 0; p < n; ++p) {
        PupilBounds B;
        std::memcpy(&B, static_cast<const char *>(bounds) + 48 * p, sizeof B);
        for (unsigned j = 0; j < m; ++j) {
            const long i = p * static_cast<long>(m) + j;
            const Splat R = lambda ? splat_point_spectral(T, D, lambda[p], pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], B, u[2 * i], u[2 * i + 1])
                                   : splat_point(T, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], B, u[2 * i], u[2 * i + 1]);
            std::memcpy(static_cast<char *>(out) + 32 * i, &R, sizeof R);
        }
    }
    return 0;
}
"""


def splat():
    """zsp_splats, called through drive_splat"""
    return host_drivers._build("splat", SPLAT)


def drive_splat(driver, cam, p, pts, bounds, u, lam=None, dispersion=None):
    """the records (n, m) of _capi.SPLAT_DTYPE the host build gives points (n,3) with their pupil-bounds records (n,) and u (n,m,2);
    lam (n,) with dispersion = cam.dispersion()"""
    info = cam.info()
    n = info["lensCount"]
    el = [np.ascontiguousarray(info["elements"][:, k], dtype=np.float32) for k in range(4)]
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(bounds)
    u = np.ascontiguousarray(u, np.float32)
    assert b.dtype == np.dtype(_capi.PUPIL_BOUNDS_DTYPE) and b.shape == (len(pts),)
    assert u.ndim == 3 and u.shape[0] == len(pts) and u.shape[2] == 2
    m = u.shape[1]
    out = np.zeros((len(pts), m), _capi.SPLAT_DTYPE)
    out["reserved"] = 0xDEAD
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    F = ctypes.c_float
    lm = None if lam is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lam, np.float32), (len(pts),)))
    dp = None if dispersion is None else np.ascontiguousarray(np.stack([dispersion["ior_d"], dispersion["cauchy_b"]], 1), np.float32)
    assert (lm is None) == (dp is None) or p["lensModel"] != _capi.RAYTRACED
    rc = driver.zsp_splats(int(p["lensModel"]), F(info["tan_fov"]), n, P(el[0]), P(el[1]), P(el[2]), P(el[3]), info["apertureElement"],
                           F(info["userApertureRadius"]), F(info["originShift"]), F(p["sensorWidth"]),
                           int(bool(p["kolbSamplingLUT"]) and len(info["lutKeys"]) > 0), len(info["lutKeys"]), int(not info["fastRunsStrict"]),
                           F(info["apertureRadius"]), F(p["focalDistance"]), int(bool(p["useDof"])), F(p.get("opticalVignettingDistance", 0.0)),
                           F(p.get("opticalVignettingRadius", 1.0)), P(dp), ctypes.c_long(len(pts)), P(pts), P(b), P(lm), ctypes.c_uint(m), P(u),
                           P(out))
    assert rc == 0, rc
    return out

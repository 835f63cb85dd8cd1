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
// The same records by the KERNEL's walk (pupil_bounds.hip) on the host: 64 lanes, lane l takes the aims l, l + 64, ... into its own
// PupilAcc, then the six rounds of the butterfly (off = 32 ... 1: every lane merges the partner l ^ off's value of before the round with
// pupil_merge), and the record is taken from lane `lane` (the kernel writes lane 0's; after the butterfly every lane holds it).
extern "C" int zpb_bounds_waves(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior, const float *aperture,
                                int apertureElement, float userApertureRadius, float originShift, float sensorWidth, int useLUT, int lutSize, int domain,
                                float apertureRadius, float focalDistance, int useDof, float ovDistance, float ovRadius, const float *disp,
                                long n, const float *pts, const float *lambda, int G, const float *window, void *out, int lane)
{
    using namespace zoic;
    if (!pupil_lattice_valid(G) || lane < 0 || lane > 63) return 1;
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
    const int shift = pupil_shift(G);
    const PupilFrame F = pupil_frame(T, G);
    for (long i = 0; i < n; ++i) {
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        PupilAcc A[64], was[64];
        for (int l = 0; l < 64; ++l)
            for (int k = 0; k < (G * G) / 64; ++k) {
                if (lambda)
                    pupil_aim(A[l], F, shift, l + 64 * k, px, py, pz, W, [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
                        return trace_back_ray_spectral(T, D, lambda[i], ox, oy, oz, dx, dy, dz, sx, sy); });
                else
                    pupil_aim(A[l], F, shift, l + 64 * k, px, py, pz, W, [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
                        return trace_back_ray(T, ox, oy, oz, dx, dy, dz, sx, sy); });
            }
        for (int off = 32; off >= 1; off >>= 1) {
            for (int l = 0; l < 64; ++l) was[l] = A[l];
            for (int l = 0; l < 64; ++l) pupil_merge(A[l], was[l ^ off]);
        }
        B[i] = pupil_record(A[lane], F, shift);
    }
    return 0;
}
"""


def pupil():
    """zpb_bounds, called through drive_pupil"""
    return host_drivers._build("pupil_bounds", PUPIL)


def drive_pupil(driver, cam, p, pts, G, window=None, lam=None, dispersion=None, wave_lane=None):
    """the records (n,) of _capi.PUPIL_BOUNDS_DTYPE the host build gives points (n,3); lam (n,) with dispersion = cam.dispersion().
    wave_lane: None, or the lane 0 ... 63 whose record zpb_bounds_waves returns: the kernel's walk and butterfly on the host"""
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
    fn, tail = (driver.zpb_bounds, ()) if wave_lane is None else (driver.zpb_bounds_waves, (int(wave_lane),))
    rc = fn(int(p["lensModel"]), F(info["tan_fov"]), n, P(el[0]), P(el[1]), P(el[2]), P(el[3]), info["apertureElement"],
                           F(info["userApertureRadius"]), F(info["originShift"]), F(p["sensorWidth"]),
                           int(bool(p["kolbSamplingLUT"]) and len(info["lutKeys"]) > 0), len(info["lutKeys"]), int(not info["fastRunsStrict"]),
                           F(info["apertureRadius"]), F(p["focalDistance"]), int(bool(p["useDof"])), F(p.get("opticalVignettingDistance", 0.0)),
                           F(p.get("opticalVignettingRadius", 1.0)), P(dp), ctypes.c_long(len(pts)), P(pts), P(lm), int(G), P(w), P(out), *tail)
    assert rc == 0, rc
    return out

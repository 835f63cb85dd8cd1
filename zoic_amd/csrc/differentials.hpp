// differentials.hpp -- traced ray differentials of the batch camera rays (zoic_ray_differentials_device,
// zoic_create_rays_arnold_differentials): the derivatives of a ray's origin and direction with respect to its screen
// sample, as Arnold reads them from AtCameraOutput (dOdx, dOdy, dDdx, dDdy).  The reference leaves dOdx / dDdx at zero and
// writes dOdy = origin, dDdy = dir for retried rays (zoic.cpp:1971-1977, "EXPERIMENTAL, I KNOW IT IS INCORRECT"); the ray
// entry points keep that for parity, these entry points trace the real thing.
//
// Definition.  For a ray with weight > 0, sx, sy its screen sample and a its ACCEPTED try (tries = bits 1-5 of the flags):
//   RAYTRACED  the accepted try starts at the sensor point o = (sx sw/2, sy sw/2, originShift), sw = sensorWidth (the y
//              component uses the width too, zoic.cpp:1853-1855), and aims at the lens point L = (Lx, Ly, originShift -
//              thickness[0]), the try's sample after the exit-pupil transform: with the LUT its scale, translation and rotation
//              (zoic.cpp:1891-1943; try 0 translates x only, :1914, retries both components, :1933), without it the sample times
//              lenses[0].aperture (:1873-1885).  The derivatives hold L FIXED while (sx, sy) move the sensor point and follow the
//              ray through every interface (signed-root sphere hit, normal, Snell as calculateTransmissionVector writes it,
//              zoic.cpp:973-1025) and the final flip (:1959).
//   THINLENS   the lens point (the output origin) is held fixed: dO = 0; dD is the derivative of normalize(p |focalDistance| -
//              origin), p = (sx tan_fov, sy tan_fov, 1), followed by the z flip (zoic.cpp:1796-1845); without DOF of normalize(p).
//   Output     dOdx = dO/dsx * dsx, dOdy = dO/dsy * dsy, likewise for D (Arnold's convention).  Rays of weight 0 (among them the
//              exhausted ones, tries 26) and every ray of lensModel NONE get +0.0 in all 12 floats.  Rays outside the exit-pupil
//              LUT (flag bit 6) are differentiated like any other, through the same fenced lookup the ray kernels used.
// This is the derivative of the path the record took -- not a finite difference, and not with the unit-square sample held
// fixed; holding L fixed makes it independent of the LUT's piecewise interpolation and of kolbSamplingLUT.
//
// The pass REPLAYS, it does not fuse: it reads the sample, the record's try count and the ray's retry stream, rebuilds L with the
// ray kernels' own STRICT device helpers (setup_ray, lens_sample, retry_direction) and traces ONE try -- the primal and two
// tangents -- without deciding anything (the record says the path passes).  The transfer arithmetic below is f32 with explicit
// FMAs and the same in every precision mode, so STRICT and FAST cameras give bitwise-equal differentials wherever their records'
// tries agree.  Transfer and refraction terms: Igehy 1999, "Tracing Ray Differentials", applied to the reference's own formulas.
//
// Out of scope (the reference's derivative fields are kept there): tiles and the per-sample zoic_camera_create_ray (the resident
// kernel, mailbox.hip), zoic_create_rays_host, zoic_frame_* / ShardedFrame and the Arnold node shim.  The records of
// zoic_create_rays_spectral_device: differentials_spectral.hpp.
//
// Host- and device-callable (ZOIC_HD): a host driver checks the tangents against finite differences
// (tests/test_differentials_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "kernels.hpp"
#include "optics.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

#if defined(__HIP_DEVICE_COMPILE__)
ZOIC_HD float diff_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }   // v_rsq_f32 / v_sqrt_f32 / v_rcp_f32: 1 ulp
ZOIC_HD float diff_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
ZOIC_HD float diff_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#else
ZOIC_HD float diff_rsqrt(float x) { return 1.0f / sqrtf(x); }
ZOIC_HD float diff_sqrt(float x) { return sqrtf(x); }
ZOIC_HD float diff_rcp(float x) { return 1.0f / x; }
#endif

ZOIC_HD float diff_dot(V3 a, V3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
ZOIC_HD V3 diff_axpy(V3 a, float s, V3 b) { return V3{fmaf(a.x, s, b.x), fmaf(a.y, s, b.y), fmaf(a.z, s, b.z)}; }   // a s + b
ZOIC_HD V3 diff_scale(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
ZOIC_HD V3 diff_neg(V3 a) { return V3{-a.x, -a.y, -a.z}; }

// tangent of v / |v| for the tangent dv of v, given u = v / |v| and inv = 1 / |v|: (dv - u (u . dv)) / |v|
ZOIC_HD V3 diff_normalize_tangent(V3 u, float inv, V3 dv) { return diff_scale(diff_axpy(u, -diff_dot(u, dv), dv), inv); }

// the 12 floats of one ray: dO/dsx, dO/dsy, dD/dsx, dD/dsy (before the dsx / dsy scale)
struct RayDifferential { V3 dOdx, dOdy, dDdx, dDdy; };

// One interface of traceThroughLensElements (zoic.cpp:1099-1158) for a ray that passes it, with the tangents (dO, dD) of both
// screen directions carried along.  Only center, radius2, sign and eta of the surface are read.
//   u = normalize(d)                                   du = (dd - u (u . dd)) / |d|
//   hit = o + u t, t = tca + sign thc (ONE signed root, zoic.cpp:986)
//   dt from the hit condition |hit - C|^2 = R^2:       dt = -w . (do + t du) / (w . u),  w = hit - C
//     (the same derivative as differentiating tca and thc, without the cancellation of two |R|-sized terms at the stop)
//   N = sign normalize(C - hit)                        dN = sign normalize'(-dhit)
//   c1 = -u . N, cs2 = eta^2 (1 - c1^2), k = eta c1 - sqrt|1 - cs2|
//                                                      dk = dc1 (eta - sgn(1 - cs2) eta^2 c1 / sqrt|1 - cs2|)
//   d' = eta u + k N                                   dd' = eta du + k dN + dk N
// (eta = ior1 / ior2, or ior1 where ior2 == 1: the branch of calculateTransmissionVector, zoic.cpp:1013, folded into Surface::eta)
ZOIC_HD void diff_interface(const Surface &S, V3 &o, V3 &d, V3 &dox, V3 &ddx, V3 &doy, V3 &ddy)
{
    const float inv = diff_rsqrt(diff_dot(d, d));
    const V3 u = diff_scale(d, inv);
    const V3 dux = diff_normalize_tangent(u, inv, ddx), duy = diff_normalize_tangent(u, inv, ddy);
    const V3 L{-o.x, -o.y, S.center - o.z};
    const float tca = diff_dot(L, u);
    const float d2 = fmaf(-tca, tca, diff_dot(L, L));
    const float thc = diff_sqrt(fabsf(S.radius2 - d2));
    const float t = fmaf(thc, S.sign, tca);
    const V3 hit = diff_axpy(u, t, o);
    const V3 w{hit.x, hit.y, hit.z - S.center};
    const float rwu = diff_rcp(diff_dot(w, u));
    const V3 px = diff_axpy(dux, t, dox), py = diff_axpy(duy, t, doy);
    const V3 dhx = diff_axpy(u, -diff_dot(w, px) * rwu, px), dhy = diff_axpy(u, -diff_dot(w, py) * rwu, py);
    // normal (zoic.cpp:999-1004; its second normalisation at :1010 is the identity on a unit vector)
    const V3 c{-hit.x, -hit.y, S.center - hit.z};
    const float invc = diff_rsqrt(diff_dot(c, c));
    const V3 nh = diff_scale(c, invc);
    const V3 N = diff_scale(nh, S.sign);
    const V3 dNx = diff_scale(diff_normalize_tangent(nh, invc, diff_neg(dhx)), S.sign);
    const V3 dNy = diff_scale(diff_normalize_tangent(nh, invc, diff_neg(dhy)), S.sign);
    // calculateTransmissionVector, zoic.cpp:1008-1025
    const float c1 = -diff_dot(u, N);
    const float dc1x = -fmaf(dux.x, N.x, fmaf(dux.y, N.y, fmaf(dux.z, N.z, diff_dot(u, dNx))));
    const float dc1y = -fmaf(duy.x, N.x, fmaf(duy.y, N.y, fmaf(duy.z, N.z, diff_dot(u, dNy))));
    const float eta = S.eta, eta2 = eta * eta;
    const float q = fmaf(eta2, c1 * c1, 1.0f - eta2);   // 1 - cs2
    const float sq = diff_sqrt(fabsf(q));
    const float k = fmaf(eta, c1, -sq);
    const float sgnq = q < 0.0f ? -1.0f : 1.0f;
    const float kk = fmaf(-sgnq * eta2 * c1, diff_rcp(sq), eta);   // dk / dc1
    const float dkx = dc1x * kk, dky = dc1y * kk;
    d = diff_axpy(N, k, diff_scale(u, eta));
    ddx = diff_axpy(N, dkx, diff_axpy(dNx, k, diff_scale(dux, eta)));
    ddy = diff_axpy(N, dky, diff_axpy(dNy, k, diff_scale(duy, eta)));
    dox = dhx; doy = dhy;
    o = hit;
}

// RAYTRACED: the accepted try from the sensor point o0 = (o0x, o0y, originShift) along d0 = L - o0 (what the ray kernels start the
// try with), L fixed: d(o0)/dsx = (halfSensor, 0, 0) = -d(d0)/dsx, likewise for sy.  surfAt(i) returns interface i (rear first).
// oOut / dOut: the traced ray after the flip (what the record holds, up to rounding).
template <class SurfAt>
ZOIC_HD RayDifferential kolb_differentials(SurfAt surfAt, int count, float halfSensor, V3 o, V3 d, V3 *oOut = nullptr, V3 *dOut = nullptr)
{
    V3 dox{halfSensor, 0.0f, 0.0f}, ddx{-halfSensor, 0.0f, 0.0f};
    V3 doy{0.0f, halfSensor, 0.0f}, ddy{0.0f, -halfSensor, 0.0f};
    for (int i = 0; i < count; ++i) {
        const Surface S = surfAt(i);
        diff_interface(S, o, d, dox, ddx, doy, ddy);
    }
    if (oOut) *oOut = diff_neg(o);
    if (dOut) *dOut = diff_neg(d);
    return RayDifferential{diff_neg(dox), diff_neg(doy), diff_neg(ddx), diff_neg(ddy)};   // zoic.cpp:1959-1961
}

// THINLENS: D = normalize(q) with the z flip; q = p |focalDistance| - origin (DOF) or p (no DOF), dq/dsx = (a, 0, 0), dq/dsy = (0, a, 0)
// with a = tan_fov |focalDistance| resp. tan_fov.  dO = 0.
ZOIC_HD RayDifferential thin_differentials(V3 q, float a)
{
    const float inv = diff_rsqrt(diff_dot(q, q));
    const V3 D = diff_scale(q, inv);
    V3 dx = diff_normalize_tangent(D, inv, V3{a, 0.0f, 0.0f});
    V3 dy = diff_normalize_tangent(D, inv, V3{0.0f, a, 0.0f});
    dx.z = dx.z * -1.0f;   // zoic.cpp:1845
    dy.z = dy.z * -1.0f;
    return RayDifferential{V3{0.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}, dx, dy};
}

// ---- launchers (differentials.hip) ------------------------------------------------------------------------------------
// model: ZOIC_THINLENS (0) or ZOIC_RAYTRACED (1).  `rays` are the records zoic_create_rays_device wrote for these samples.
// Batch form: d_samples = n x (sx, sy, lensx, lensy), d_out = n x 12 floats (dOdx, dOdy, dDdx, dDdy) scaled by dsx / dsy.
int launch_ray_differentials(int model, const KolbTable &kolb, const ThinTable &thin, const BokehTables &bokeh, const float *d_samples,
                             const uint32_t *d_rng, uint64_t rayBase, uint64_t n, const RayRecord *rays, float dsx, float dsy,
                             float *d_out, void *stream);
// Arnold rows: d_inputs7 = n AtCameraInput rows (sx sy dsx dsy lensx lensy time: each row's own dsx / dsy), d_out21 = n whole
// AtCameraOutput rows -- origin, dir and weight exactly as launch_expand_outputs writes them, the four derivative fields traced.
int launch_expand_outputs_differentials(int model, const KolbTable &kolb, const ThinTable &thin, const BokehTables &bokeh,
                                        const float *d_inputs7, uint64_t rayBase, uint64_t n, const RayRecord *rays, float *d_out21,
                                        void *stream);

}  // namespace zoic

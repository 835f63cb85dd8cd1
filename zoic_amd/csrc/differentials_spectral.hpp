// differentials_spectral.hpp -- traced ray differentials of the rays zoic_create_rays_spectral_device made
// (zoic_ray_differentials_spectral_device): differentials.hpp's tangent trace with every interface's eta taken at the ray's own
// wavelength (spectral.hpp's Cauchy indices), and optionally one more tangent, the derivative of the path with respect to the
// wavelength.
//
// Definition.  For a record of weight > 0 whose wavelength lambda is valid (spectral_valid):
//   Screen tangents   dOdx, dOdy, dDdx, dDdy exactly as differentials.hpp defines them (the accepted try, the lens point L held
//                     fixed), through diff_interface itself, with eta_i(lambda) in place of Surface::eta.
//   Wavelength tangent  dO/dlambda, dD/dlambda per NANOMETRE of the same try with the sensor point AND L held fixed: the start
//                     tangents are zero, and interface i adds the source term of its eta,
//                         dn_i/dlambda = -2 B_i / lambda^3  (0 for air and behind the last interface)
//                         deta = (dn1 n2 - n1 dn2) / n2^2
//                     to the transfer terms of diff_interface applied to this tangent (du, dhit, dN, dc1).  With
//                     q = 1 - eta^2 (1 - c1^2), k = eta c1 - sqrt|q|, d' = eta u + k N:
//                         dq  = -2 eta deta (1 - c1^2) + 2 eta^2 c1 dc1
//                         dk  = deta c1 + eta dc1 - sgn(q) dq / (2 sqrt|q|)
//                             = dc1 (eta - sgn(q) eta^2 c1 / sqrt|q|) + deta (c1 + sgn(q) eta (1 - c1^2) / sqrt|q|)
//                         dd' = deta u + eta du + dk N + k dN
//                     followed by the final flip (zoic.cpp:1959) like the other tangents.  dsx / dsy never scale it.
//                     This tangent is traced in F64, primal included, from the try's f32 start and the f32 table: a lens is
//                     achromatised by making its crown and flint contributions cancel, so the tangent is what remains of a sum 25
//                     (PETZVAL) to 46 (TESSAR) times its size, and every contribution inherits the relative rounding of the path it
//                     is evaluated on.  In f32 that left 7e-6 of the tangent (median; 3e-4 at the 99.9th percentile), 27 - 83 times
//                     the screen tangents' error; in f64 the result is the f32 rounding of the exact tangent.  The indices are the
//                     Cauchy model in f64 on the table's f32 entries (n_d, B), lambda_d = 587.5618.
//   Index             dl = spectral_dl(lambda) once per ray; per interface spectral_iors and spectral_eta -- the forward kernels' own
//                     f32 operations.  eta follows the STRICT rule (one correctly rounded division) in every precision mode, so
//                     STRICT and FAST cameras give bitwise-equal results wherever their records' tries agree; at lambda_d, and on a
//                     lens without V-numbers (every B = 0) at any wavelength, the screen tangents are kolb_differentials' bit for bit.
//   THINLENS          ignores the wavelength: thin_differentials' 12 floats, +0.0 in the six more.
//   Zeros             weight 0 (among them the forward call's rejected records, flags 0x80), an invalid wavelength HERE whatever the
//                     record says, lensModel NONE: +0.0 in every float.
// Nothing is decided in this pass (no TIR test, no clip): the record says the path passes.
//
// Host- and device-callable (ZOIC_HD): tests/test_differentials_spectral_cpu.py drives a host build against f64 central differences.
#pragma once
#include "differentials.hpp"
#include "spectral.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// the 12 floats of differentials.hpp and the wavelength tangent (per nm; zeros where it was not asked for)
struct SpectralDifferential { RayDifferential screen; V3 dOdl, dDdl; };

// The wavelength tangent of the try (o, d) at lambda, after the final flip: an f64 trace of its own beside the f32 one of the
// screen tangents (the definition above has the reason).  surfAt / W / count as kolb_differentials_spectral.
struct D3 { double x, y, z; };
ZOIC_HD double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ZOIC_HD D3 daxpy(D3 a, double s, D3 b) { return D3{a.x * s + b.x, a.y * s + b.y, a.z * s + b.z}; }   // a s + b
ZOIC_HD D3 dscale(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
ZOIC_HD D3 dnormalize_tangent(D3 u, double inv, D3 dv) { return dscale(daxpy(u, -ddot(u, dv), dv), inv); }

template <class SurfAt, class WP>
ZOIC_HD void kolb_wavelength_tangent(SurfAt surfAt, WP W, int count, float lambdaF, V3 o0, V3 d0, V3 &dOdl, V3 &dDdl)
{
    const double lambda = static_cast<double>(lambdaF);
    const double dl = 1.0 / (lambda * lambda) - 1.0 / (kLambdaD * kLambdaD);
    const double dnScale = -2.0 / (lambda * lambda * lambda);
    D3 o{o0.x, o0.y, o0.z}, d{d0.x, d0.y, d0.z};
    D3 dol{0.0, 0.0, 0.0}, ddl{0.0, 0.0, 0.0};
    for (int i = 0; i < count; ++i) {
        const Surface S = surfAt(i);
        ZOIC_SPEC_PIN(W);
        const double b1 = static_cast<double>(W->cauchyB[i]), b2 = (i + 1 < count) ? static_cast<double>(W->cauchyB[i + 1]) : 0.0;
        const double n1 = static_cast<double>(W->iorD[i]) + b1 * dl;
        const double n2 = (i + 1 < count) ? static_cast<double>(W->iorD[i + 1]) + b2 * dl : 1.0;
        const double eta = n1 / n2;
        const double deta = (b1 * n2 - n1 * b2) * dnScale / (n2 * n2);
        const double center = static_cast<double>(S.center), radius2 = static_cast<double>(S.radius2), sign = static_cast<double>(S.sign);
        // the interface of diff_interface, one tangent
        const double inv = 1.0 / sqrt(ddot(d, d));
        const D3 u = dscale(d, inv);
        const D3 dul = dnormalize_tangent(u, inv, ddl);
        const D3 L{-o.x, -o.y, center - o.z};
        const double tca = ddot(L, u);
        const double d2 = ddot(L, L) - tca * tca;
        const double t = tca + sqrt(fabs(radius2 - d2)) * sign;
        const D3 hit = daxpy(u, t, o);
        const D3 w{hit.x, hit.y, hit.z - center};
        const D3 pl = daxpy(dul, t, dol);
        const D3 dhl = daxpy(u, -ddot(w, pl) / ddot(w, u), pl);
        const D3 c{-hit.x, -hit.y, center - hit.z};
        const double invc = 1.0 / sqrt(ddot(c, c));
        const D3 nh = dscale(c, invc);
        const D3 N = dscale(nh, sign);
        const D3 dNl = dscale(dnormalize_tangent(nh, invc, D3{-dhl.x, -dhl.y, -dhl.z}), sign);
        const double c1 = -ddot(u, N);
        const double dc1l = -(ddot(dul, N) + ddot(u, dNl));
        const double q = 1.0 - eta * eta * (1.0 - c1 * c1);
        const double sq = sqrt(fabs(q));
        const double k = eta * c1 - sq;
        const double sgnq = q < 0.0 ? -1.0 : 1.0;
        const double kk = eta - sgnq * eta * eta * c1 / sq;                    // dk / dc1
        const double ke = c1 + sgnq * eta * (1.0 - c1 * c1) / sq;              // dk / deta
        const double dkl = dc1l * kk + deta * ke;
        ddl = daxpy(N, dkl, daxpy(dNl, k, daxpy(u, deta, dscale(dul, eta))));
        d = daxpy(N, k, dscale(u, eta));
        dol = dhl;
        o = hit;
    }
    dOdl = V3{static_cast<float>(-dol.x), static_cast<float>(-dol.y), static_cast<float>(-dol.z)};   // zoic.cpp:1959-1961
    dDdl = V3{static_cast<float>(-ddl.x), static_cast<float>(-ddl.y), static_cast<float>(-ddl.z)};
}

// kolb_differentials at the wavelength lambda (valid: the caller checked).  surfAt(i): interface i (center, radius2, sign are read);
// W: the camera's dispersion table (spectral.hpp: `const SpectralTable *` on the host, the kernel-argument pointer on the device).
template <bool CHROMATIC, class SurfAt, class WP>
ZOIC_HD SpectralDifferential kolb_differentials_spectral(SurfAt surfAt, WP W, int count, float lambda, float halfSensor, V3 o, V3 d,
                                                         V3 *oOut = nullptr, V3 *dOut = nullptr)
{
    const float dl = spectral_dl(lambda);
    const V3 oStart = o, dStart = d;
    V3 dox{halfSensor, 0.0f, 0.0f}, ddx{-halfSensor, 0.0f, 0.0f};
    V3 doy{0.0f, halfSensor, 0.0f}, ddy{0.0f, -halfSensor, 0.0f};
    for (int i = 0; i < count; ++i) {
        Surface S = surfAt(i);
        ZOIC_SPEC_PIN(W);
        float ior1, ior2;
        spectral_iors(W, count, i, dl, ior1, ior2);
        S.eta = spectral_eta(ior1, ior2);
        diff_interface(S, o, d, dox, ddx, doy, ddy);
    }
    if (oOut) *oOut = diff_neg(o);
    if (dOut) *dOut = diff_neg(d);
    SpectralDifferential g{RayDifferential{diff_neg(dox), diff_neg(doy), diff_neg(ddx), diff_neg(ddy)},   // zoic.cpp:1959-1961
                           V3{0.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}};
    if constexpr (CHROMATIC) kolb_wavelength_tangent(surfAt, W, count, lambda, oStart, dStart, g.dOdl, g.dDdl);
    return g;
}

// ---- launcher (spectral_differentials.hip) -------------------------------------------------------------------------------
// launch_ray_differentials for the records of launch_kolb_spectral / launch_spectral_reject: d_lambda = n f32 (nm); d_chromatic:
// nullptr, or n x 6 floats (dO/dlambda, dD/dlambda).  model: ZOIC_THINLENS (0) or ZOIC_RAYTRACED (1).
int launch_ray_differentials_spectral(int model, const KolbTable &kolb, const SpectralTable &spec, const ThinTable &thin,
                                      const BokehTables &bokeh, const float *d_samples, const float *d_lambda, const uint32_t *d_rng,
                                      uint64_t rayBase, uint64_t n, const RayRecord *rays, float dsx, float dsy, float *d_out,
                                      float *d_chromatic, void *stream);

}  // namespace zoic

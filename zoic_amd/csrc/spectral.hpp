// spectral.hpp -- rays traced at a wavelength of their own (zoic_create_rays_spectral_device): the dispersion model and the
// per-ray interface arithmetic of the STRICT spectral trace.
//
// Model.  Each medium behind interface i (trace order, rear first: zo_lenses / LensSystem::rows after prepare()) has a
// two-term Cauchy index through its d-line index n_d (the table's ior after the 0 -> 1.0 fix, zoic.cpp:937-940) and its
// Abbe number V_d (the fifth column of a prescription, zoic.cpp:524, or zoic_camera_set_abbe_numbers):
//     n_i(lambda) = n_d,i + B_i (1/lambda^2 - 1/lambda_d^2)
//     B_i = (n_d,i - 1) / (V_i (1/lambda_F^2 - 1/lambda_C^2))     in f64, rounded once to f32 (host: cauchy_b)
//     B_i = 0 where n_d,i == 1 (air), V_i is not finite or V_i <= 0 (4-column prescriptions: V = 0)
// so n(lambda_F) - n(lambda_C) = (n_d - 1) / V: the Abbe number's own definition.  Per ray, in f32 with one rounding per
// operator (no fused multiply-add):  dl = 1/(lambda lambda) - kInvD2,  n_i = n_d,i + B_i dl.  At lambda_d, dl == 0 and n_i == n_d,i
// exactly; air stays 1.0 at every wavelength.  Each interface then applies the reference's own rules to the per-ray indices:
// eta = ior2 == 1 ? ior1 : ior1 / ior2 (zoic.cpp:1013), total internal reflection possible iff ior1 > ior2 (zoic.cpp:1019).
// The exit-pupil LUT, the focus (originShift), the focal-length rescale and the bokeh tables stay those of the d-line: the
// camera is focused at lambda_d, and other colours show longitudinal chromatic aberration.
//
// Wavelengths are nanometres; a ray whose wavelength is outside [360, 830] or NaN is rejected: +0.0 origin and direction,
// weight 0, flags == kSpectralRejected, no counter.
//
// Host- and device-callable (ZOIC_HD): tests/test_spectral_cpu.py checks the host build against a numpy restatement.
#pragma once
#include <cmath>
#include <cstdint>

#include "kernels.hpp"
#include "optics.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr double kLambdaD = 587.5618, kLambdaF = 486.1327, kLambdaC = 656.2725;   // nm: He d, H F, H C lines
constexpr float kLambdaMin = 360.0f, kLambdaMax = 830.0f;
constexpr uint32_t kSpectralRejected = 0x80u;   // flag bit 7: wavelength rejected

// Per-medium dispersion of one camera, trace order; a kernel argument by value (wave-uniform: scalar loads).
struct SpectralTable {
    int32_t count;                    // == KolbTable::lensCount
    int32_t pad[3];
    float iorD[kMaxSurfaces];         // n_d after the 0 -> 1.0 fix
    float cauchyB[kMaxSurfaces];      // B_i (nm^2)
    float invAbsRR[kMaxSurfaces];     // 1 / (|R| R) of interface i (FAST: krScale = eta invAbsRR)
};

// B of one medium (host, f64, one rounding to f32)
inline float cauchy_b(float iorD, float abbe)
{
    if (iorD == 1.0f || !std::isfinite(abbe) || !(abbe > 0.0f)) return 0.0f;
    const double span = 1.0 / (kLambdaF * kLambdaF) - 1.0 / (kLambdaC * kLambdaC);
    return static_cast<float>(static_cast<double>(iorD - 1.0f) / (static_cast<double>(abbe) * span));
}

constexpr float kLambdaD32 = 587.5618f;   // the d-line in f32: the wavelength of a pass that is given none (spectral_dl gives exactly 0 there)

ZOIC_HD bool spectral_valid(float lambda) { return lambda >= kLambdaMin && lambda <= kLambdaMax; }   // false for NaN

// 1/lambda^2 - 1/lambda_d^2 in f32 (kInvD2 by the same f32 operations)
ZOIC_HD float spectral_dl(float lambda)
{
    const float invD2 = 1.0f / (kLambdaD32 * kLambdaD32);
    return 1.0f / (lambda * lambda) - invD2;
}

ZOIC_HD float spectral_ior(float iorD, float b, float dl)
{
    const float t = b * dl;   // a multiply, then an add: two roundings (contraction is off)
    return iorD + t;
}

// Table access of the traces below: WP is `const SpectralTable *` on the host; on the device a pointer into the kernel-argument
// segment (address space 4: scalar loads), re-derived per interface behind an empty asm so that the compiler neither hoists the
// loads of every interface out of the kernel's loops into SGPRs nor copies the by-value tables to scratch (fast_optics.hpp
// launder_table has the story).
#if defined(__HIP_DEVICE_COMPILE__)
#define ZOIC_SPEC_PIN(p) asm volatile("" : "+s"(p))
#else
#define ZOIC_SPEC_PIN(p) ((void)0)
#endif

// the per-ray pair of interface i: ior1 = n_i, ior2 = n_{i+1}, 1.0 behind the last interface (zoic.cpp:1137-1143)
template <class WP>
ZOIC_HD void spectral_iors(WP W, int count, int i, float dl, float &ior1, float &ior2)
{
    ior1 = spectral_ior(W->iorD[i], W->cauchyB[i], dl);
    ior2 = (i + 1 < count) ? spectral_ior(W->iorD[i + 1], W->cauchyB[i + 1], dl) : 1.0f;
}
ZOIC_HD float spectral_eta(float ior1, float ior2) { return (ior2 == 1.0f) ? ior1 : ior1 / ior2; }   // zoic.cpp:1013
ZOIC_HD bool spectral_tir_possible(float ior1, float ior2) { return ior1 > ior2; }                   // zoic.cpp:1019

// trace_lens_strict (optics.hpp) with the per-ray eta / tirPossible of every interface: the reference's arithmetic, operation for
// operation; (o, d) are left as the reference leaves them on every exit path.  SP: pointer to the KolbTable's Surface array.
// observe(i, ior1, ior2, eta, c1) is called at every interface the ray refracts at (after the clip and the total-reflection test): it
// reads the trace's values and feeds nothing back (transmittance.hpp rides along here); the empty observer compiles away.
struct NoInterfaceObserver {
    ZOIC_HD void operator()(int, float, float, float, float) const {}
};
template <class SP, class WP, class Observe>
ZOIC_HD bool trace_lens_spectral_strict_observed(SP surf, WP W, int count, float dl, V3 &o, V3 &d, uint32_t &tirCount, Observe &observe)
{
    for (int ii = 0; ii < count; ++ii) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int i = __builtin_amdgcn_readfirstlane(ii);
#else
        const int i = ii;
#endif
        ZOIC_SPEC_PIN(surf);
        ZOIC_SPEC_PIN(W);
        const float center = surf[i].center, radius2 = surf[i].radius2, sign = surf[i].sign, housing2 = surf[i].housing2;
        V3 u = normalize3(d);
        V3 L{0.0f - o.x, 0.0f - o.y, center - o.z};
        float tca = dot3(L, u);
        float d2 = dot3(L, L) - (tca * tca);
        if (d2 > radius2) return false;
        float thc = ZOIC_SQRT_RN(fabsf(radius2 - d2));
        float t = tca + thc * sign;
        V3 hit{o.x + u.x * t, o.y + u.y * t, o.z + u.z * t};
        float h2 = hit.x * hit.x + hit.y * hit.y;
        if (h2 > housing2) return false;
        V3 nrm = normalize3(V3{0.0f - hit.x, 0.0f - hit.y, center - hit.z});
        nrm = V3{nrm.x * sign, nrm.y * sign, nrm.z * sign};
        o = hit;
        float ior1, ior2;
        spectral_iors(W, count, i, dl, ior1, ior2);
        const float eta = spectral_eta(ior1, ior2);
        V3 N = normalize3(nrm);
        float c1 = -dot3(u, N);
        float cs2 = static_cast<float>(static_cast<double>(eta * eta) * (1.0 - static_cast<double>(c1 * c1)));
        if (spectral_tir_possible(ior1, ior2) && cs2 > 1.0f) {
            ++tirCount;
            return false;
        }
        observe(i, ior1, ior2, eta, c1);
        float k = static_cast<float>(static_cast<double>(eta * c1) - sqrt(fabs(1.0 - static_cast<double>(cs2))));
        d = V3{u.x * eta + N.x * k, u.y * eta + N.y * k, u.z * eta + N.z * k};
    }
    return true;
}
template <class SP, class WP>
ZOIC_HD bool trace_lens_spectral_strict(SP surf, WP W, int count, float dl, V3 &o, V3 &d, uint32_t &tirCount)
{
    NoInterfaceObserver none;
    return trace_lens_spectral_strict_observed(surf, W, count, dl, o, d, tirCount, none);
}

// ---- launcher (spectral.hip) ----------------------------------------------------------------------------------------------
// RAYTRACED rays at per-ray wavelengths: d_lambda = n f32 (nm).  mode: 0 STRICT, 1 / 2 FAST (decision-safe; a clip inside a guard
// band is re-taken in the reference's arithmetic).  Records and counters as launch_kolb_rays.
int launch_kolb_spectral(const KolbTable &table, const SpectralTable &spec, const BokehTables &bokeh, const float *d_samples,
                         const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, RayRecord *out,
                         DeviceCounters *d_counters, int mode, void *stream);
// The other lens models ignore the wavelength: their records come from launch_thin_rays; this pass then rejects the rows whose
// wavelength is invalid (zeros, flags kSpectralRejected) and takes back the counter bump the thin-lens kernel gave them
// (countsRays: the model counts every ray -- THINLENS with depth of field).
int launch_spectral_reject(const float *d_lambda, uint64_t n, RayRecord *out, DeviceCounters *d_counters, bool countsRays, void *stream);

}  // namespace zoic

// transmittance.hpp -- the Fresnel transmittance of a traced ray (zoic_ray_transmittance_device): the share of unpolarised light that
// the interfaces of a lens let through along the path of one try, bare or with a single-layer coating per interface.
//
// Definition.  Inputs per column: one try's start (o, d), a wavelength lambda (nm, valid: spectral_valid), the interfaces, the
// dispersion table (spectral.hpp) and a film table.  T = prod_i T_i over the interfaces of the path that the STRICT spectral interface
// arithmetic takes from that start: trace_lens_spectral_strict's operations, operation for operation (at lambda_d: trace_lens_strict's)
// -- the observer below rides along with that one body and feeds nothing back into it.
//   Per interface  ci = |c1|;  (n1, n2) = spectral_iors(...);  ct = sqrt|1 - eta^2 (1 - c1^2)| in f32 on the trace's f32 eta and c1.
//   Uncoated       rs = (n1 ci - n2 ct) / (n1 ci + n2 ct);  rp = (n1 ct - n2 ci) / (n1 ct + n2 ci);  T_i = 1 - (rs^2 + rp^2) / 2:
//                  unpolarised light, no absorption.
//   Coated         a film of index nc, a quarter wave thick at lambda0 (thickness lambda0 / (4 nc)); it does not disperse.
//                  cc = sqrt(1 - (n1 / nc)^2 (1 - ci^2)), the cosine inside the film.  Fresnel amplitudes a (medium 1 -> film) and b
//                  (film -> medium 2), for each polarisation, in the sign convention of rs / rp above:
//                      a_s = (n1 ci - nc cc) / (n1 ci + nc cc)      b_s = (nc cc - n2 ct) / (nc cc + n2 ct)
//                      a_p = (n1 cc - nc ci) / (n1 cc + nc ci)      b_p = (nc ct - n2 cc) / (nc ct + n2 cc)
//                  c2b = cos(pi (lambda0 / lambda) cc), the round trip's phase;
//                  R = (a^2 + b^2 + 2 a b c2b) / (1 + a^2 b^2 + 2 a b c2b);  T_i = 1 - (R_s + R_p) / 2.
//   Equal media    n1 == n2 at that wavelength: T_i = 1.0 exactly, the film entry is ignored.  The stop is one (air on both sides).
//   Evanescent     where (n1 / nc)^2 (1 - ci^2) > 1 the film carries no wave: the ray takes the uncoated formula at that interface.
//   No path        the replayed path misses a sphere, is clipped or is totally reflected: T = +0.0.  Possible only for records of the
//                  unchecked FAST mode or inputs that do not match the records.  A path that passes has T > 0.
//   Film table     per interface (trace order) the film's index and lambda0 (nm); index 0: uncoated.
//
// Arithmetic.  f32, contraction off, only correctly rounded operations: + - x /, ZOIC_SQRT_RN, ZOIC_RCP_RN and explicit fmaf; fabsf and
// floorf are exact.  The cosine is the polynomial film_cospi below after an exact range reduction (no library cos).  So the host build
// and the kernel give the same bits, the way traceback_jacobian.hpp does.
//
// Host- and device-callable (ZOIC_HD): tests/test_transmittance_cpu.py drives a host build against an f64 numpy restatement
// (tests/transmittance_ref.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "spectral.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// Per-interface coatings of one camera, trace order; a kernel argument by value (wave-uniform: scalar loads).
struct FilmTable {
    int32_t count;                    // == KolbTable::lensCount
    int32_t pad[3];
    float index[kMaxSurfaces];        // nc; 0: uncoated
    float lambda0[kMaxSurfaces];      // nm: the film is a quarter wave thick there
};

// cos(pi x) for x >= 0 (the film's x = (lambda0 / lambda) cc lies in [0, 2.31] for a lambda0 in the visible range).  Reduction: y = x - 2 m
// with the integer m = floor(x / 2 + 1/4) is exact (a difference of two multiples of ulp(x) that is smaller than x), y in [-1/2, 3/2];
// for y > 1/2, z = y - 1 (exact: Sterbenz) and cos(pi y) = -cos(pi z).  Then the degree-5 polynomial in z^2 that interpolates cos(pi z)
// at the Chebyshev nodes of z^2 in [0, 1/4], by Horner with fmaf.  Largest error against f64 cos(pi x) on [0, 2.31]: 1.1e-7 (the
// rounding of the evaluation; the polynomial itself is good to 3e-9).
ZOIC_HD float film_cospi(float x)
{
    const float m = floorf(x * 0.5f + 0.25f);
    const float y = x - 2.0f * m;
    const bool flip = y > 0.5f;
    const float z = flip ? y - 1.0f : y;
    const float t = z * z;
    float p = -0.024395931512117386f;
    p = fmaf(p, t, 0.23493707180023193f);
    p = fmaf(p, t, -1.335211992263794f);
    p = fmaf(p, t, 4.058709144592285f);
    p = fmaf(p, t, -4.934802055358887f);
    p = fmaf(p, t, 1.0f);
    return flip ? -p : p;
}

// the reflectance of two amplitudes a, b a phase apart (Airy's sum of the film's multiple reflections, no absorption)
ZOIC_HD float film_reflectance(float a, float b, float c2b)
{
    const float ab = a * b;
    const float cross = (2.0f * ab) * c2b;
    return ((a * a + b * b) + cross) / ((1.0f + ab * ab) + cross);
}

// T_i of one interface: media n1 -> n2 (n1 != n2), ci = |cos i|, ct = cos t; nc == 0: uncoated
ZOIC_HD float interface_transmittance(float n1, float n2, float ci, float ct, float nc, float lambda0, float lambda)
{
    if (nc != 0.0f) {
        const float q = n1 / nc;
        const float s2 = (q * q) * (1.0f - ci * ci);
        if (!(s2 > 1.0f)) {
            const float cc = ZOIC_SQRT_RN(1.0f - s2);
            const float c2b = film_cospi((lambda0 / lambda) * cc);
            const float as = (n1 * ci - nc * cc) / (n1 * ci + nc * cc), bs = (nc * cc - n2 * ct) / (nc * cc + n2 * ct);
            const float ap = (n1 * cc - nc * ci) / (n1 * cc + nc * ci), bp = (nc * ct - n2 * cc) / (nc * ct + n2 * cc);
            return 1.0f - (film_reflectance(as, bs, c2b) + film_reflectance(ap, bp, c2b)) * 0.5f;
        }
    }
    const float rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct);
    const float rp = (n1 * ct - n2 * ci) / (n1 * ct + n2 * ci);
    return 1.0f - (rs * rs + rp * rp) * 0.5f;
}

// The observer of trace_lens_spectral_strict_observed that multiplies the T_i up.  FP: `const FilmTable *` on the host, the
// kernel-argument pointer on the device (read like the dispersion table: ZOIC_SPEC_PIN).
template <class FP>
struct TransmittanceObserver {
    FP F;
    float lambda;
    float T;
    ZOIC_HD void operator()(int i, float n1, float n2, float eta, float c1)
    {
        FP film = F;   // a copy per interface: the pinned pointer is not carried round the trace's loop, whose lanes leave it one by one
        ZOIC_SPEC_PIN(film);
        const float nc = film->index[i], lambda0 = film->lambda0[i];
        if (n1 == n2) return;
        const float ci = fabsf(c1);
        const float ct = ZOIC_SQRT_RN(fabsf(1.0f - (eta * eta) * (1.0f - c1 * c1)));
        T = T * interface_transmittance(n1, n2, ci, ct, nc, lambda0, lambda);
    }
};

// T of the try (o, d) at lambda (valid: the caller checked); SP, WP as trace_lens_spectral_strict
template <class SP, class WP, class FP>
ZOIC_HD float path_transmittance(SP surf, WP W, FP F, int count, float lambda, V3 o, V3 d)
{
    TransmittanceObserver<FP> obs{F, lambda, 1.0f};
    uint32_t tir = 0;
    const bool ok = trace_lens_spectral_strict_observed(surf, W, count, spectral_dl(lambda), o, d, tir, obs);
    return ok ? obs.T : 0.0f;
}

// ---- launcher (transmittance.hip) ----------------------------------------------------------------------------------------
// The records of launch_kolb_rays / launch_kolb_spectral (k == 1) or launch_kolb_hero (k >= 2), n x k sample-major, -> n x k floats.
// d_lambda: n x k f32 (nm), or nullptr with k == 1: the d-line.  model: ZOIC_THINLENS (0) or ZOIC_RAYTRACED (1).  Nothing but d_out is
// written.  d_stacks: the camera's StackTable (coating_stack.hpp) on the device where an interface has a multilayer stack (the
// stack-aware kernel), nullptr otherwise.
struct StackTable;
int launch_ray_transmittance(int model, const KolbTable &kolb, const SpectralTable &spec, const FilmTable &film, const BokehTables &bokeh,
                             const float *d_samples, const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k,
                             const RayRecord *rays, float *d_out, void *stream, const StackTable *d_stacks = nullptr);

}  // namespace zoic

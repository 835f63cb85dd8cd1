// coating_stack.hpp -- multilayer coatings (zoic_camera_set_coating_stacks): per interface an optional stack of 1 to kCoatingMaxLayers
// homogeneous, loss-free, non-dispersive layers, priced by the characteristic-matrix (Abeles) method at the ray's own angle and
// wavelength, for both polarisations.  transmittance.hpp knows a bare interface and one quarter-wave film; this is the coating lenses
// really carry, and it reaches every consumer of interface_transmittance at once: the forward transmittance, the ghosts' weights and
// the trace-back / splat transmittance.
//
// Definition.  Media n1 -> n2 (n1 the side the ray comes from), ci = |cos i| in n1, ct = cos t in n2, wavelength lambda (nm), and the
// interface's L layers (index n_j, physical thickness d_j in nm) IN THE ORDER THE RAY MEETS THEM.
//   Layer cosine   cc_j = sqrt(1 - (n1 / n_j)^2 (1 - ci^2)): the cc of transmittance.hpp's film.
//   Phase          x_j = 2 n_j d_j cc_j / lambda;  c_j = cos(pi x_j), s_j = sin(pi x_j).
//   Admittance     eta_j = n_j cc_j for s and n_j / cc_j for p; eta0 from (n1, ci), etas from (n2, ct).
//   Matrix         M = [[A, iB], [iC, D]] from the identity; a loss-free stack keeps A, B, C, D real.  Per layer a = c_j, b = s_j / eta_j,
//                  c = eta_j s_j, d = c_j and  A' = A a - B c,  B' = A b + B d,  C' = C a + D c,  D' = D d - C b.
//   R, T_i         R = ((eta0 A - etas D)^2 + (eta0 etas B - C)^2) / ((eta0 A + etas D)^2 + (eta0 etas B + C)^2);
//                  T_i = 1 - (R_s + R_p) / 2.
//   No stack       layers == 0: the interface is priced exactly as before, by its film entry or bare (interface_transmittance).
//   Equal media    n1 == n2: T_i = 1.0f exactly, the stack is ignored -- decided by the callers before they come here, as for the film.
//   Evanescent     where any layer has (n1 / n_j)^2 (1 - ci^2) >= 1 (no wave in it, or cc_j == 0) the interface takes the bare formula:
//                  interface_transmittance with nc == 0, its bits.  (The single film's rule with > made >=, for stacks only.)
//   Range          T_i is finite and in [0, 1] for every ci, ct in [0, 1], +0 included -- see the three points below.
//
// How the range is kept.
//   p without a division by a cosine.  The p matrix is run on the DUAL admittance eta' = cos / n (eta0' = ci / n1, eta_j' = cc_j / n_j,
//   etas' = ct / n2).  Exchanging E and H turns M into [[D, iC], [iB, A]] and every eta into 1 / eta; put into R and multiplied through
//   by (eta0 etas)^2 that is the same quotient, so R_p is unchanged while ci = 0 or ct = 0 only make an admittance 0.  The one
//   division left is b = s_j / eta_j by a LAYER's cosine, and the evanescent rule has cc_j >= 2^-12 (1 - s2 is at least one ulp of 1).
//   No overflow.  b <= 4 x 2^12 = 2^14 and c <= 4, so one layer multiplies the largest of |A|, |B|, |C|, |D| by less than 2^15.  After
//   every layer, a matrix whose largest entry has reached 2^16 is multiplied by 2^-16: exact (a power of two; an entry that drops
//   into the denormals is 2^-100 of its neighbours) and without effect on R, which is homogeneous of degree 0 in M.  So the largest entry
//   stays below 2^16 at every layer's start, below 2^31 inside one, and the terms of R (admittances <= 4) below 2^41 squared once.
//   The quotient.  AD + BC = 1, so in exact arithmetic the numerator is the denominator less 4 eta0 etas and R <= 1; rounding can
//   exceed that by an ulp, and eta0 = etas = 0 with C = 0 makes 0 / 0.  R is taken as 1 where the denominator is not positive (grazing
//   incidence reflects everything) and otherwise as the smaller of the quotient and 1.  Both terms being squares, R >= 0.
//
// Arithmetic.  As transmittance.hpp: f32, contraction off, only + - x /, ZOIC_SQRT_RN and explicit fmaf; fabsf, floorf, comparisons
// and selects are exact.  film_cospi as it is, and film_sinpi below with the same range reduction.  The setter's limits (index <= 4,
// thickness <= 1000 nm, lambda >= 360 nm) bound x by 2 x 4 x 1000 / 360 = 22.3, not the single film's 2.31.  The reduction is exact
// there as it is everywhere below 2^23: m = floor(x / 2 + 1/4) <= 11 is an integer, 2 m a multiple of ulp(x) for x >= 1, and y = x - 2 m
// is a multiple of ulp(x) no larger than x, hence a float; where x / 2 + 1/4 rounds up to an integer y falls short of -1/2 by less than
// 2^-21, which the polynomials do not notice.  Largest error against f64 on 10^5 points of [0, 22.3]: cos 1.0e-7, sin 1.7e-7
// (tests/test_coating_stacks_cpu.py).  So the host build and the kernels give the same bits.
//
// Table.  32 x (count + 8 indices + 8 thicknesses) = 2176 bytes: it does not fit in the 4 KB of kernel arguments beside the tables the
// kernels already take (device_pass.hpp), so the camera keeps it in a device buffer next to its GhostTable, with a host copy for the
// host calls.  Interfaces in trace order (rear first), each interface's layers in the order a FORWARD ray (rear to front) meets them;
// a ray going the other way -- the trace-back, a ghost's middle leg -- walks them backwards.  The interface index is wave-uniform in
// all three consumers, so the layer count and the layer loop are uniform and the table is read with scalar loads.
// zoic_camera_set_coating_stacks uploads the table with a blocking copy, ordered against the caller's work exactly as
// zoic_camera_update orders its copy of the GhostTable: both are setters of the camera, which the threading contract allows only
// while no call on the camera is in flight, and both have landed when the call returns.
//
// Kernels.  The plain kernels are launched as before whenever no interface of the camera has a stack; the stack-aware instances
// (coating policy `const StackTable *` in place of NoStacks) only otherwise.
//
// Host- and device-callable (ZOIC_HD): tests/test_coating_stacks_cpu.py drives a host build against an f64 complex transfer-matrix
// restatement (tests/coating_stack_ref.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "transmittance.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr int kCoatingMaxLayers = 8;

// The stacks of one camera: trace order, layers in the order a forward ray meets them.
struct StackLayer { float index, thickness; };            // thickness in nm; one 8-byte scalar load
struct StackTable {
    int32_t layers[kMaxSurfaces];                         // 0: no stack, the film entry (or bare) holds
    StackLayer layer[kMaxSurfaces][kCoatingMaxLayers];
};

// The coating policy of the kernels and calls that know no stacks: coated_transmittance is interface_transmittance.
struct NoStacks {};

ZOIC_HD int stack_uniform(int j)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(j);   // wave-uniform: the table entry is a scalar load
#else
    return j;
#endif
}

// ZOIC_SQRT_RN for a layer's 1 - s2, which lies in [2^-24, 1]: inside exact_math.hpp's guard range, so the device takes the lean
// sequence without the guard's branch (a divergent branch in the layer loop costs a saved exec mask); the same bits.
ZOIC_HD float stack_sqrt(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return sqrt_rn_lean(x);
#else
    return sqrtf(x);
#endif
}

// sin(pi x) for x >= 0: film_cospi's reduction (y = x - 2 m in [-1/2, 3/2]; for y > 1/2, z = y - 1 and sin(pi y) = -sin(pi z)), then
// z times the degree-5 polynomial in z^2 that interpolates sin(pi z) / z at the Chebyshev nodes of z^2 in [0, 1/4] (good to 3e-11).
ZOIC_HD float film_sinpi(float x)
{
    const float m = floorf(x * 0.5f + 0.25f);
    const float y = x - 2.0f * m;
    const bool flip = y > 0.5f;
    const float z = flip ? y - 1.0f : y;
    const float t = z * z;
    float p = -0.007028304040431976f;
    p = fmaf(p, t, 0.08205035328865051f);
    p = fmaf(p, t, -0.5992521643638611f);
    p = fmaf(p, t, 2.5501632690429688f);
    p = fmaf(p, t, -5.167712688446045f);
    p = fmaf(p, t, 3.1415927410125732f);
    const float s = p * z;
    return flip ? -s : s;
}

// both at once for the layer loop: one reduction, film_cospi's and film_sinpi's operations on it, hence their bits
ZOIC_HD void film_sincospi(float x, float &sn, float &cs)
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
    float q = -0.007028304040431976f;
    q = fmaf(q, t, 0.08205035328865051f);
    q = fmaf(q, t, -0.5992521643638611f);
    q = fmaf(q, t, 2.5501632690429688f);
    q = fmaf(q, t, -5.167712688446045f);
    q = fmaf(q, t, 3.1415927410125732f);
    const float sign = flip ? -1.0f : 1.0f;   // (a product with +-1 is the negation's bits)
    cs = p * sign;
    sn = (q * z) * sign;
}

// one polarisation's matrix, [[A, iB], [iC, D]]
struct StackMatrix { float A, B, C, D; };

ZOIC_HD void stack_layer(StackMatrix &M, float c, float s, float eta)
{
    const float b = s / eta, g = eta * s;
    const float A = M.A * c - M.B * g, B = M.A * b + M.B * c;
    const float C = M.C * c + M.D * g, D = M.D * c - M.C * b;
    const float big = fmaxf(fmaxf(fabsf(A), fabsf(B)), fmaxf(fabsf(C), fabsf(D)));
    const float k = big >= 65536.0f ? 0x1p-16f : 1.0f;   // (a power of two: exact, and R does not see it)
    M.A = A * k; M.B = B * k; M.C = C * k; M.D = D * k;
}

ZOIC_HD float stack_reflectance(const StackMatrix &M, float eta0, float etas)
{
    const float u = eta0 * M.A, v = etas * M.D, w = (eta0 * etas) * M.B, z = M.C;
    const float num = (u - v) * (u - v) + (w - z) * (w - z);
    const float den = (u + v) * (u + v) + (w + z) * (w + z);
    const float R = num / den;   // (0 / 0 is selected away: no branch)
    return (den > 0.0f && R < 1.0f) ? R : 1.0f;
}

// T_i of interface i through its L >= 1 layers; forward: the ray travels rear to front (the table's order).  false: a layer is
// evanescent, the caller takes the bare formula.  i and L are wave-uniform on the device, and a lane with an evanescent layer stays in
// the loop on a cosine of 1 (its result is dropped): the loop has no divergent exit and costs no saved exec masks.
template <class KP>
ZOIC_HD bool stack_transmittance(KP K, int i, int L, bool forward, float n1, float n2, float ci, float ct, float lambda, float &T)
{
    StackMatrix S{1.0f, 0.0f, 0.0f, 1.0f}, P{1.0f, 0.0f, 0.0f, 1.0f};
    const float sin2 = 1.0f - ci * ci;
    float worst = 0.0f;   // the largest (n1 / n_j)^2 sin^2 i of the layers
    const StackLayer *y = K->layer[i] + (forward ? 0 : L - 1);   // one moving pointer and a count: the loop's whole scalar state
#pragma clang loop unroll(disable)
    for (int l = L; l > 0; --l, y += forward ? 1 : -1) {
        const StackLayer Y = *y;
        const float nj = Y.index, dj = Y.thickness;
        const float q = n1 / nj;
        const float s2 = (q * q) * sin2;
        const bool wave = s2 < 1.0f;
        worst = fmaxf(worst, s2);   // (a register of the lane's own, not a lane mask carried round the loop)
        const float cc = stack_sqrt(wave ? 1.0f - s2 : 1.0f);
        const float x = (((2.0f * nj) * dj) * cc) / lambda;
        float c, s;
        film_sincospi(x, s, c);
        stack_layer(S, c, s, nj * cc);
        stack_layer(P, c, s, cc / nj);   // the dual admittance
    }
    const float Rs = stack_reflectance(S, n1 * ci, n2 * ct);
    const float Rp = stack_reflectance(P, ci / n1, ct / n2);
    T = 1.0f - (Rs + Rp) * 0.5f;
    return worst < 1.0f;
}

// T_i of interface i (trace order, n1 != n2) under a coating policy: the stack where the interface has one, else its film entry or bare
ZOIC_HD float coated_transmittance(NoStacks, int, bool, float n1, float n2, float ci, float ct, float nc, float lambda0, float lambda)
{
    return interface_transmittance(n1, n2, ci, ct, nc, lambda0, lambda);
}

template <class KP>
ZOIC_HD float coated_transmittance(KP K, int i, bool forward, float n1, float n2, float ci, float ct, float nc, float lambda0, float lambda)
{
    const int ii = stack_uniform(i);
    const int L = stack_uniform(K->layers[ii]);
    if (L > 0) {
        float T;
        const bool wave = stack_transmittance(K, ii, L, forward, n1, n2, ci, ct, lambda, T);
        const float bare = interface_transmittance(n1, n2, ci, ct, 0.0f, 0.0f, lambda);   // (a select, not a branch: two divisions)
        return wave ? T : bare;
    }
    return interface_transmittance(n1, n2, ci, ct, nc, lambda0, lambda);
}

// transmittance.hpp's observer and path under a coating policy (KP = NoStacks: TransmittanceObserver's own operations)
template <class FP, class KP>
struct CoatedTransmittanceObserver {
    FP F;
    KP K;
    float lambda;
    float T;
    ZOIC_HD void operator()(int i, float n1, float n2, float eta, float c1)
    {
        FP film = F;
        ZOIC_SPEC_PIN(film);
        const float nc = film->index[i], lambda0 = film->lambda0[i];
        if (n1 == n2) return;
        const float ci = fabsf(c1);
        const float ct = ZOIC_SQRT_RN(fabsf(1.0f - (eta * eta) * (1.0f - c1 * c1)));
        T = T * coated_transmittance(K, i, true, n1, n2, ci, ct, nc, lambda0, lambda);
    }
};

template <class SP, class WP, class FP, class KP>
ZOIC_HD float path_transmittance(SP surf, WP W, FP F, KP K, int count, float lambda, V3 o, V3 d)
{
    CoatedTransmittanceObserver<FP, KP> obs{F, K, lambda, 1.0f};
    uint32_t tir = 0;
    const bool ok = trace_lens_spectral_strict_observed(surf, W, count, spectral_dl(lambda), o, d, tir, obs);
    return ok ? obs.T : 0.0f;
}

// Host: whether any interface of the table has a stack (the launchers' choice of kernel)
inline bool stacks_in_use(const StackTable &K, int count)
{
    for (int i = 0; i < count && i < kMaxSurfaces; ++i)
        if (K.layers[i] > 0) return true;
    return false;
}

}  // namespace zoic

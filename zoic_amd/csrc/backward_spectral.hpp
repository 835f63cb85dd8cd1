// backward_spectral.hpp -- the two backward lens paths at a wavelength per item: zoic_trace_back_rays_spectral_device /
// zoic_trace_back_ray_spectral (traceback.hpp's trace) and zoic_project_points_spectral_device / zoic_project_point_spectral
// (reverse.hpp's projection).  The forward path traces at a wavelength per ray (spectral.hpp); a light tracer, a splatter or a
// bidirectional integrator that connects to that camera has to come back through the same glass: a spectral record traced back at
// the d-line lands on a sample that is off by the lens's chromatic aberration, and a point splatted in blue and in red has to land
// on two different pixels (lateral colour).
//
// Definition.  Everything is traceback.hpp's / reverse.hpp's, with one change: the ratio of the two media at every interface.
//   Index      The medium behind interface i (trace order, rear first) has n_i(lambda) = spectral_ior(n_d,i, B_i, spectral_dl(lambda)):
//              spectral.hpp's functions as they are (f32, one rounding per operator: the forward kernels' own sequence), n_d and B the
//              values zoic_camera_get_dispersion reports (a zoic_camera_set_abbe_numbers override included).  The medium in front of
//              the front element is exactly 1.0f.  dl is computed once per item.
//   Ratio      Every interface takes the true ratio of its two media, as the d-line tables do (fill_traceback_table,
//              fill_reverse_table): trace-back eta = n_front / n_rear; projection etaF = n_rear / n_front (towards the front) and
//              etaR = n_front / n_rear (towards the rear).  Each is ONE correctly rounded f32 division (div_rn below).  An
//              interface's rear medium is the next interface's front medium, so a pass costs one spectral_ior and one division per
//              interface on top of the d-line pass.
//   Unchanged  Geometry, housings, the stop limit, the sensor plane (originShift), the focal-length rescale, the LUT flag, the
//              domain gate, the cap test, the projection's paraxial first guess (it only seeds the search) and every arithmetic step
//              that does not read an index: the camera is focused at 587.5618 nm, as on the forward side.
//   At the d-line (kLambdaD32)   spectral_dl is exactly 0, every n_i is n_d,i, every ratio is the host table's own division: Ps and flags
//              equal the d-line calls' bit for bit, for every input (the same templates run, traceback.hpp trace_back_ray and
//              reverse.hpp project_point, with another source of eta).
//   Rejected   A wavelength outside [360, 830] nm, or NaN, rejects that item alone, before anything else is looked at (as the
//              forward path's 0x80): Ps = (+0, +0), bit 0 clear, reason kTbWavelength (8) / kRevWavelength (6).  THINLENS and NONE
//              cameras ignore the wavelength apart from that: their answers are the d-line calls'.
//
// Division.  div_rn(a, b) is the language's a / b on both sides: IEEE-754 division, not a reciprocal-plus-residual sequence of our own.
// Host: divss.  Device: the library is compiled with -fno-fast-math and hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, under
// which clang lowers an f32 `/` to the AMDGPU backend's correctly rounded sequence (the one LLVM specifies as 0.5 ulp), visible in the
// two kernels' ISA:
//     v_div_scale_f32 (x2)   numerator and denominator scaled by powers of two, exactly, so that no intermediate leaves the normal range
//     v_rcp_f32              y0 = 1/b to 1 ulp
//     two FMAs               y1 = y0 + y0 (1 - b y0): one Newton step
//     three FMAs             q0 = a y1;  q1 = q0 + y1 (a - b q0): the residual a - b q0 is exact in one FMA
//     one FMA, v_div_fmas    q = q1 + y1 (a - b q1): again an exact residual, so this last sum is rounded ONCE
//     v_div_fixup_f32        the scaling undone; 0, inf, NaN and denormal results patched
// Why the last rounding is the right one is Markstein's theorem (P. Markstein, "Computation of elementary functions on the IBM RISC
// System/6000 processor", 1990): with y1 within an ulp of 1/b and q1 within an ulp of a/b, RN(q1 + y1 (a - b q1)) = RN(a / b).  This
// file adds nothing to that argument and depends on no property of its own operands -- refractive indices in [1, ~2.5], where neither
// the scaling nor the fix-up does anything.  spectral_dl's `1.0f / x` has relied on the same lowering in the forward kernels (whose
// host and device bits are compared by tests/test_spectral_gpu.py).  The check that does not rest on the argument:
// tests/test_backward_spectral_gpu.py compares device and host bit for bit on five lenses at wavelengths uniform in [360, 830] nm,
// i.e. every ratio through the results it feeds.  No f64 on the device.
//
// Tables.  The d-line tables stay as they are (by-value kernel arguments); BackwardDispersion adds, per interface and in the same
// front-to-rear order, the pair (n_d, B) of the medium BEHIND it: one aligned 8-byte entry, one scalar load (the interface index is
// wave-uniform).
//
// Host- and device-callable (ZOIC_HD): tests/test_backward_spectral_cpu.py drives the host build against an f64 restatement.
#pragma once
#include <cstdint>

#include "reverse.hpp"
#include "spectral.hpp"
#include "traceback.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

ZOIC_HD float div_rn(float a, float b) { return a / b; }   // correctly rounded on host and device: see "Division" above

struct alignas(8) BwdMedium {   // one 8-byte entry: one scalar load per interface
    float iorD;      // n_d of the medium behind the interface
    float cauchyB;   // its B (nm^2)
};

// Front-to-rear order (entry j is trace-order index count-1-j), as TraceBackTable::surf and ReverseTable::surf.
struct BackwardDispersion {
    BwdMedium med[kMaxSurfaces];
};

ZOIC_HD float bwd_ior(const BwdMedium *med, int j, float dl)
{
    const BwdMedium m = med[j];   // the whole entry at once
    return spectral_ior(m.iorD, m.cauchyB, dl);
}

// traceback.hpp's Medium: front to rear, the rear index of one interface is the front index of the next
struct TbSpectral {
    const BwdMedium *med;
    float dl;
    float nFront;   // 1.0f in front of the front element
    ZOIC_HD float eta(int j, const TbSurface &)
    {
        const float nRear = bwd_ior(med, j, dl);
        const float e = div_rn(nFront, nRear);
        nFront = nRear;
        return e;
    }
};

// reverse.hpp's Medium: every pass starts at the stop, with the index of the medium in front of it (computed once per item)
struct RevSpectral {
    const BwdMedium *med;
    float dl;
    float nStop;   // the medium between interface stop-1 and the stop (1.0f when the stop is the front interface)
    float carry;
    ZOIC_HD void at_stop() { carry = nStop; }
    ZOIC_HD float eta_front(int j, const RevSurface &)   // towards the front: n_rear / n_front
    {
        const float nRear = carry;
        const float nFront = j > 0 ? bwd_ior(med, j - 1, dl) : 1.0f;
        carry = nFront;
        return div_rn(nRear, nFront);
    }
    ZOIC_HD float eta_rear(int j, const RevSurface &)    // towards the rear: n_front / n_rear
    {
        const float nFront = carry;
        const float nRear = bwd_ior(med, j, dl);
        carry = nRear;
        return div_rn(nFront, nRear);
    }
};

// the trace-back of one ray at its wavelength (nm): returns the flag word, writes sx, sy
ZOIC_HD uint32_t trace_back_ray_spectral(const TraceBackTable &T, const BackwardDispersion &D, float lambda, float ox, float oy, float oz,
                                         float dx, float dy, float dz, float &sx, float &sy)
{
    if (!spectral_valid(lambda)) {
        sx = 0.0f; sy = 0.0f;
        return kTbWavelength << kTbReasonShift;
    }
    return trace_back_ray(T, ox, oy, oz, dx, dy, dz, sx, sy, TbSpectral{D.med, spectral_dl(lambda), 1.0f});
}

// the projection of one point at its wavelength (nm): returns the flag word, writes sx, sy
ZOIC_HD uint32_t project_point_spectral(const ReverseTable &T, const BackwardDispersion &D, float lambda, float px, float py, float pz,
                                        float &sx, float &sy)
{
    if (!spectral_valid(lambda)) {
        sx = 0.0f; sy = 0.0f;
        return kRevWavelength << kRevReasonShift;
    }
    const float dl = spectral_dl(lambda);
    const int stop = rev_uniform(T.stop);
    const float nStop = (T.model == 1 && stop > 0) ? bwd_ior(D.med, stop - 1, dl) : 1.0f;
    return project_point(T, px, py, pz, sx, sy, RevSpectral{D.med, dl, nStop, nStop});
}

// Host: the dispersion of a camera's lens (SpectralTable, trace order) in the backward tables' front-to-rear order
inline void fill_backward_dispersion(BackwardDispersion &D, const SpectralTable &W)
{
    for (int j = 0; j < kMaxSurfaces; ++j) D.med[j] = BwdMedium{1.0f, 0.0f};
    const int count = W.count < kMaxSurfaces ? W.count : kMaxSurfaces;
    for (int j = 0; j < count; ++j) {
        const int i = count - 1 - j;
        D.med[j] = BwdMedium{W.iorD[i], W.cauchyB[i]};
    }
}

// ---- launchers (traceback.hip, reverse.hip) ------------------------------------------------------------------------------
// As launch_trace_back / launch_project_points, with d_lambda = n f32 wavelengths (nm, 4-byte aligned).  Asynchronous on `stream`.
int launch_trace_back_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda, uint64_t n,
                               float *d_screen, uint32_t *d_flags, void *stream);
int launch_project_points_spectral(const ReverseTable &T, const BackwardDispersion &D, const float *d_points, const float *d_lambda,
                                   uint64_t n, float *d_screen, uint32_t *d_flags, void *stream);

}  // namespace zoic

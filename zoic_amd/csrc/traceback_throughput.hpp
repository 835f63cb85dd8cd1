// traceback_throughput.hpp -- the Fresnel transmittance of a ray traced BACK through the lens (zoic_trace_back_transmittance_device,
// zoic_trace_back_ray_transmittance, zoic_splat_transmittance_device, zoic_splat_point_transmittance and their _spectral forms).  The
// forward side accounts for the light the glass reflects away (transmittance.hpp: a bare DOUBLE_GAUSS passes 0.59); the backward calls
// returned geometry only, so a light tracer, a splatter or a bidirectional integrator that connects to the camera through them saw a
// loss-free lens, inconsistent with its own forward pass by a factor that depends on field, wavelength and coating.  This is the
// missing factor: the T of the very path that trace_back_ray_spectral takes.
//
// Definition.  The ray is traced back exactly as trace_back_ray_spectral traces it: traceback.hpp's tb_trace with backward_spectral.hpp's
// TbSpectral medium, both untouched.  A d-line call is the spectral call at kLambdaD32, where backward_spectral.hpp guarantees the
// d-line call's Ps and flags bit for bit.  A rider (tb_trace's Tangents slot) multiplies T = prod_j T_j up over the interfaces, front
// to rear (entry j is trace-order index count-1-j):
//   n1, n2     n1 is the front-side index: exactly 1.0f in front of the front element, otherwise the previous interface's n2;
//              n2 = bwd_ior(med, j, dl).  These are the values TbSpectral forms eta = n1 / n2 from: the rider keeps its own copy of
//              (med, dl, nFront) and repeats the one multiply and add, which gives the same bits (and which a compiler merges).
//   ci, ct     ci = |cosi|; ct is the trace's own sqrt(k2), the refracted cosine (k2 = 1 - eta^2 (1 - cosi^2)).  No second root.
//   Film       entry count-1-j of the FilmTable that the forward call reads (trace order), read at the call.
//   Equal      n1 == n2 (the stop: air on both sides): T_j = 1.0f exactly, the film entry is ignored.
//   Otherwise  T_j = interface_transmittance(n1, n2, ci, ct, nc, lambda0, lambda) of transmittance.hpp, unchanged, its evanescent-film
//              rule included.  T = T * T_j, in trace order, from 1.0f.
//   Result     a traced ray (kTbTraced): T.  Anything else -- every refusal reason, a wavelength outside [360, 830] nm or NaN -- +0.0f.
//              THINLENS with depth of field has no interface: 1.0f where traced, +0.0f otherwise.  NONE and THINLENS without: +0.0f.
//   Ps, flags  the trace-back's own bits for every input: the rider reads the trace's values and feeds nothing back.
//
// Reciprocity.  A loss-free interface reflects the same share from either side (rs, rp only change sign when (n1, ci) and (n2, ct)
// change places; the film's Airy sum is symmetric in a and b, and the film's own cosine cc is the same from both sides by Snell), so
// the backward T of a forward record equals the forward T of its start, to the rounding of the two traces.
//
// Arithmetic.  As transmittance.hpp and traceback.hpp: f32, contraction off, correctly rounded operations only, so the host build and
// the kernels give the same bits.
//
// Splat side.  The same T for the rays that the fused splat call traces: splat.hpp's aim and ray construction repeated operation for
// operation (splat_aim, dir = P - A, splat_plane), then the trace above -- without the Jacobian's 24 tangent registers.  A point with
// an empty box (count == 0 or kPbSome clear) traces nothing and gets +0.0f.
//
// Host- and device-callable (ZOIC_HD): tests/test_traceback_throughput_cpu.py drives the host build against an f64 restatement.
#pragma once
#include <cstdint>

#include "backward_spectral.hpp"
#include "coating_stack.hpp"
#include "splat.hpp"
#include "traceback.hpp"
#include "transmittance.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// The rider: tb_trace's Tangents.  FP: `const FilmTable *` on the host, a pointer into the kernel-argument segment on the device.
// interface() is called once per interface the ray refracts at, front to rear, so the rider counts them itself; the count is the same
// in every lane that is still tracing.  KP: the coating policy (coating_stack.hpp): NoStacks, or a pointer to the camera's StackTable,
// whose layers this ray, going front to rear, meets backwards.
template <class FP, class KP = NoStacks>
struct TbThroughput {
    const BwdMedium *med;
    FP film;
    float dl, lambda;
    float nFront;   // 1.0f in front of the front element
    float T;        // 1.0f before the first interface
    int j;          // the next interface, front to rear
    int count;
    KP stacks;

    ZOIC_HD void line(float, float, float) {}
    ZOIC_HD void thin(const TraceBackTable &, float, float) {}
    ZOIC_HD void seed(float, float, float) {}
    ZOIC_HD void interface(float, float, float, float, float, float cosi, float, float sk, float, float, float, float)
    {
        const int jj = tb_uniform(j);
        const int i = count - 1 - jj;   // the film table is in trace order
        const float n1 = nFront, n2 = bwd_ior(med, jj, dl);
        const float nc = film->index[i], lambda0 = film->lambda0[i];
        nFront = n2;
        j = jj + 1;
        if (n1 == n2) return;
        T = T * coated_transmittance(stacks, i, false, n1, n2, fabsf(cosi), sk, nc, lambda0, lambda);
    }
    ZOIC_HD void sensor(const TraceBackTable &, float, float, float, float, float, float, float) {}
};

// the trace-back of one ray at its wavelength (nm) with its transmittance: returns the flag word, writes sx, sy and T
template <class FP, class KP = NoStacks>
ZOIC_HD uint32_t trace_back_ray_throughput(const TraceBackTable &T, const BackwardDispersion &D, FP film, float lambda, float ox, float oy,
                                           float oz, float dx, float dy, float dz, float &sx, float &sy, float &t, KP K = KP{})
{
    t = 0.0f;
    if (!spectral_valid(lambda)) {
        sx = 0.0f; sy = 0.0f;
        return kTbWavelength << kTbReasonShift;
    }
    const float dl = spectral_dl(lambda);
    TbSpectral M{D.med, dl, 1.0f};
    TbThroughput<FP, KP> G{D.med, film, dl, lambda, 1.0f, 1.0f, 0, T.count, K};
    const uint32_t f = tb_trace(T, ox, oy, oz, dx, dy, dz, sx, sy, M, G);
    if ((f & kTbTraced) != 0u) t = G.T;
    return f;
}

// One splat's T: splat_of's box test, aim and ray (splat.hpp), then the trace above
template <class FP, class KP = NoStacks>
ZOIC_HD float splat_throughput(const TraceBackTable &T, const BackwardDispersion &D, FP film, float lambda, float z, float px, float py,
                               float pz, float lox, float loy, float hix, float hiy, uint32_t count, uint32_t boxFlags, float u0, float u1,
                               KP K = KP{})
{
    if (count == 0u || (boxFlags & kPbSome) == 0u) return 0.0f;
    const float ax = splat_aim(lox, hix, u0), ay = splat_aim(loy, hiy, u1);
    const float dx = px - ax, dy = py - ay, dz = pz - z;
    float sx, sy, t;
    (void)trace_back_ray_throughput(T, D, film, lambda, px, py, pz, dx, dy, dz, sx, sy, t, K);
    return t;
}

// ---- launchers (traceback_throughput.hip) ----------------------------------------------------------------------------------------
// d_rays = n 32-byte zoic_ray records (16-byte aligned); d_lambda = n f32 wavelengths (nm) or nullptr: the d-line; d_out = n floats;
// d_screen = n x 2 floats (8-byte aligned) or nullptr; d_flags = n uint32 or nullptr.  Asynchronous on `stream`.  d_stacks (both
// launchers): the camera's StackTable on the device where an interface has a stack (the stack-aware kernels), nullptr otherwise.
int launch_trace_back_throughput(const TraceBackTable &T, const BackwardDispersion &D, const FilmTable &F, const void *d_rays,
                                 const float *d_lambda, uint64_t n, float *d_out, float *d_screen, uint32_t *d_flags, void *stream,
                                 const StackTable *d_stacks = nullptr);
// d_points, d_bounds, d_u as launch_splat_points; d_lambda = n f32 (one per point) or nullptr: the d-line; d_out = n x m floats.
int launch_splat_throughput(const TraceBackTable &T, const BackwardDispersion &D, const FilmTable &F, const float *d_points,
                            const void *d_bounds, const float *d_lambda, uint64_t n, uint32_t m, const float *d_u, float *d_out, void *stream,
                            const StackTable *d_stacks = nullptr);

}  // namespace zoic

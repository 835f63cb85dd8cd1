// traceback.hip -- the batch trace-back (traceback.hpp), at a wavelength per ray (backward_spectral.hpp) and with its Jacobian
// (traceback_jacobian.hpp): four kernels, one camera ray per lane.
//
// Mapping: the launch shape and the one-item-per-lane walk of device_pass.hpp.  The TraceBackTable (and, spectral, the BackwardDispersion) arrives
// by value as a kernel argument: the interface loop's index is wave-uniform, so every table entry is one 16-byte scalar load (the
// dispersion entry: one 8-byte load).  No LDS, no scratch.  A lane reads its 32-byte record as two 16-byte loads (a wave's 2 KiB are
// contiguous; the compiler narrows the second to the 8 bytes that are used) and, spectral, one more coalesced dword, its wavelength
// (48 bytes per ray moved against 44); runs the trace -- one pass over the interfaces, a lane whose ray has ended waits for the wave's
// loop; spectral: dl once, and per interface one index (a multiply and an add) and one division on top of the d-line trace -- and
// writes one float2 and, if asked, one flag word.  The Jacobian kernels carry the four tangents in 24 registers and write 48 more
// bytes of J as three 16-byte stores (a wave's 3 KiB are contiguous).
#include <hip/hip_runtime.h>

#include "device_pass.hpp"
#include "traceback_jacobian.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// the walk of the four kernels: trace(i, ox, oy, oz, dx, dy, dz, sx, sy) returns ray i's flag word
template <class Trace>
__device__ __forceinline__ void tb_walk(const float4 *__restrict__ rays, uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                        Trace trace)
{
    for_each_item(n, [&](uint64_t i) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];   // ox oy oz dx | dy dz weight flags
        float sx, sy;
        const uint32_t f = trace(i, a.x, a.y, a.z, a.w, b.x, b.y, sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    });
}

__device__ __forceinline__ void store_jacobian(float4 *__restrict__ jac, uint64_t i, const float *J)
{
    jac[3u * i] = make_float4(J[0], J[1], J[2], J[3]);
    jac[3u * i + 1u] = make_float4(J[4], J[5], J[6], J[7]);
    jac[3u * i + 2u] = make_float4(J[8], J[9], J[10], J[11]);
}

}  // namespace

// budget (all four): 0 scratch, 0 spills, 0 LDS; the spectral trace-back at most 64 VGPRs (8 waves per SIMD)
__global__ __launch_bounds__(kPassBlock) void trace_back_kernel(const TraceBackTable T, const float4 *__restrict__ rays, uint64_t n,
                                                              float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    tb_walk(rays, n, screen, flags, [&](uint64_t, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray(T, ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

__global__ __launch_bounds__(kPassBlock) void trace_back_spectral_kernel(const TraceBackTable T, const BackwardDispersion D,
                                                                       const float4 *__restrict__ rays, const float *__restrict__ lambda,
                                                                       uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    tb_walk(rays, n, screen, flags, [&](uint64_t i, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray_spectral(T, D, lambda[i], ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

__global__ __launch_bounds__(kPassBlock) void trace_back_jacobian_kernel(const TraceBackTable T, const float4 *__restrict__ rays, uint64_t n,
                                                                       float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                                                       float4 *__restrict__ jac)
{
    tb_walk(rays, n, screen, flags, [&](uint64_t i, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        float J[12];
        const uint32_t f = trace_back_ray_jacobian(T, ox, oy, oz, dx, dy, dz, sx, sy, J);
        store_jacobian(jac, i, J);
        return f;
    });
}

__global__ __launch_bounds__(kPassBlock) void trace_back_jacobian_spectral_kernel(const TraceBackTable T, const BackwardDispersion D,
                                                                                const float4 *__restrict__ rays,
                                                                                const float *__restrict__ lambda, uint64_t n,
                                                                                float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                                                                float4 *__restrict__ jac)
{
    tb_walk(rays, n, screen, flags, [&](uint64_t i, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        float J[12];
        const uint32_t f = trace_back_ray_jacobian_spectral(T, D, lambda[i], ox, oy, oz, dx, dy, dz, sx, sy, J);
        store_jacobian(jac, i, J);
        return f;
    });
}

int launch_trace_back(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(trace_back_kernel, pass_grid(n), stream, T, static_cast<const float4 *>(d_rays),
                       n, reinterpret_cast<float2 *>(d_screen), d_flags);
}

int launch_trace_back_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda, uint64_t n,
                               float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(trace_back_spectral_kernel, pass_grid(n), stream, T, D,
                       static_cast<const float4 *>(d_rays), d_lambda, n, reinterpret_cast<float2 *>(d_screen), d_flags);
}

int launch_trace_back_jacobian(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian,
                               void *stream)
{
    if (n == 0) return 0;
    return launch_pass(trace_back_jacobian_kernel, pass_grid(n), stream, T,
                       static_cast<const float4 *>(d_rays), n, reinterpret_cast<float2 *>(d_screen), d_flags,
                       reinterpret_cast<float4 *>(d_jacobian));
}

int launch_trace_back_jacobian_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda,
                                        uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(trace_back_jacobian_spectral_kernel, pass_grid(n), stream, T, D,
                       static_cast<const float4 *>(d_rays), d_lambda, n, reinterpret_cast<float2 *>(d_screen), d_flags,
                       reinterpret_cast<float4 *>(d_jacobian));
}

}  // namespace zoic

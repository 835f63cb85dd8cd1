// reverse.hip -- the batch reverse projection (reverse.hpp) and the same at a wavelength per point (backward_spectral.hpp): two
// kernels, one point per lane.
//
// Mapping: the launch shape and the one-item-per-lane walk of device_pass.hpp.  The ReverseTable (and, spectral, the BackwardDispersion)
// arrives by value as a kernel argument: the interface loops' index is wave-uniform, so every table read is a scalar load (the
// dispersion entry: one 8-byte load).  No LDS, no scratch.  A lane reads its packed float3 (three dword loads; a wave's 768 bytes are
// contiguous) and, spectral, one more coalesced dword, its wavelength; runs the search of project_point -- the lanes of a wave loop
// until the last of them has converged; spectral: dl and the index in front of the stop once, and in every pass of the search one
// index and one division per interface on top of the d-line pass -- and writes one float2 and, if asked, one flag word.
#include <hip/hip_runtime.h>

#include "backward_spectral.hpp"
#include "device_pass.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// the walk of the two kernels: project(i, px, py, pz, sx, sy) returns point i's flag word
template <class Project>
__device__ __forceinline__ void rev_walk(const float *__restrict__ points, uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                         Project project)
{
    for_each_item(n, [&](uint64_t i) {
        const float *p = points + i * 3u;
        float sx, sy;
        const uint32_t f = project(i, p[0], p[1], p[2], sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    });
}

}  // namespace

// budget (both): 0 scratch, 0 spills; the spectral projection at most 64 VGPRs (8 waves per SIMD)
__global__ __launch_bounds__(kPassBlock) void project_points_kernel(const ReverseTable T, const float *__restrict__ points, uint64_t n,
                                                                   float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    rev_walk(points, n, screen, flags, [&](uint64_t, float px, float py, float pz, float &sx, float &sy) {
        return project_point(T, px, py, pz, sx, sy);
    });
}

__global__ __launch_bounds__(kPassBlock) void project_points_spectral_kernel(const ReverseTable T, const BackwardDispersion D,
                                                                            const float *__restrict__ points, const float *__restrict__ lambda,
                                                                            uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    rev_walk(points, n, screen, flags, [&](uint64_t i, float px, float py, float pz, float &sx, float &sy) {
        return project_point_spectral(T, D, lambda[i], px, py, pz, sx, sy);
    });
}

int launch_project_points(const ReverseTable &T, const float *d_points, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(project_points_kernel, pass_grid(n), stream, T, d_points, n,
                       reinterpret_cast<float2 *>(d_screen), d_flags);
}

int launch_project_points_spectral(const ReverseTable &T, const BackwardDispersion &D, const float *d_points, const float *d_lambda,
                                   uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(project_points_spectral_kernel, pass_grid(n), stream, T, D, d_points,
                       d_lambda, n, reinterpret_cast<float2 *>(d_screen), d_flags);
}

}  // namespace zoic

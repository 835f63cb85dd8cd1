// splat.hip -- the batch lens splats (splat.hpp), d-line and at a wavelength per point: two kernels (an instance per lens model), one
// splat per lane.
//
// Mapping: the launch shape of device_pass.hpp, whose lanes walk the n m splats with a grid stride (a 64-bit index).  Splat i belongs
// to point p = i / m; the lane takes that quotient once, in 32 bits (its first index is below kPassGridCap x kPassBlock = 2^19), and then steps p and the remainder by the stride's own quotient and remainder, which are wave-uniform:
// no 64-bit division anywhere.  The TraceBackTable (and, spectral, the BackwardDispersion) arrives by value as a kernel argument, so
// the interface loop keeps its scalar table loads, as in traceback.hip.  A lane loads its point (12 bytes), the box row and the
// count / flags row of the point's pupil-bounds record (16 bytes each; the middle row, the blur spot's box, is not read) and, spectral,
// the point's wavelength: with m aims per point, m neighbouring lanes read the same lines.  u is one 8-byte load per lane, a wave's
// 512 bytes contiguous.  The lane carries the Jacobian trace's 24 tangent registers plus the aim, and writes its 32-byte record as two
// 16-byte stores (a wave's 2 KiB are contiguous).  A lane whose box is empty skips the trace under the exec mask and stores the
// kSpNoBox record; no lane returns before its store.  No atomics, no LDS, no scratch, no random numbers; nothing is read or written
// past n m.
#include <hip/hip_runtime.h>

#include "device_pass.hpp"
#include "splat.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// the grid-stride walk of both kernels: trace(p, ox, oy, oz, dx, dy, dz, sx, sy, J) returns the flag word of one ray from point p
template <class Trace>
__device__ __forceinline__ void sp_walk(const TraceBackTable &T, const float *__restrict__ points, const float4 *__restrict__ bounds, uint64_t total,
                                        uint32_t m, const float2 *__restrict__ u, float4 *__restrict__ splats, Trace trace)
{
    const float z = splat_plane(T);
    const uint32_t stride = gridDim.x * static_cast<uint32_t>(kPassBlock);   // <= 2^19
    const uint32_t first = blockIdx.x * static_cast<uint32_t>(kPassBlock) + threadIdx.x;
    const uint32_t stepP = stride / m, stepJ = stride % m;                  // wave-uniform
    uint64_t p = first / m;
    uint32_t j = first % m;
    for (uint64_t i = first; i < total; i += stride) {
        const float px = points[3u * p], py = points[3u * p + 1u], pz = points[3u * p + 2u];
        const float4 box = bounds[3u * p], tail = bounds[3u * p + 2u];     // aim[4] | count lattice flags reserved
        const float2 uu = u[i];
        const Splat S = splat_of(z, px, py, pz, box.x, box.y, box.z, box.w, __float_as_uint(tail.x), __float_as_uint(tail.z), uu.x, uu.y,
                                 [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, float *J) {
                                     return trace(p, ox, oy, oz, dx, dy, dz, sx, sy, J);
                                 });
        splats[2u * i] = make_float4(S.sx, S.sy, S.ax, S.ay);
        splats[2u * i + 1u] = make_float4(S.area, S.angle, __uint_as_float(S.flags), __uint_as_float(S.reserved));
        // i + stride = (p + stepP) m + (j + stepJ), and j + stepJ < 2 m
        p += stepP;
        if (j >= m - stepJ) { j -= m - stepJ; ++p; }
        else j += stepJ;
    }
}

}  // namespace

// The lens model is a template parameter (traceback.hpp assume_model / model_instance).
// budget (all six): 0 scratch, 0 spills, 0 LDS
template <int kModel>
__global__ __launch_bounds__(kPassBlock) void splat_kernel(const TraceBackTable T, const float *__restrict__ points, const float4 *__restrict__ bounds,
                                                         uint64_t total, uint32_t m, const float2 *__restrict__ u, float4 *__restrict__ splats)
{
    assume_model<kModel>(T);
    sp_walk(T, points, bounds, total, m, u, splats,
            [&](uint64_t, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, float *J) {
                return trace_back_ray_jacobian(T, ox, oy, oz, dx, dy, dz, sx, sy, J);
            });
}

template <int kModel>
__global__ __launch_bounds__(kPassBlock) void splat_spectral_kernel(const TraceBackTable T, const BackwardDispersion D, const float *__restrict__ points,
                                                                  const float4 *__restrict__ bounds, const float *__restrict__ lambda,
                                                                  uint64_t total, uint32_t m, const float2 *__restrict__ u,
                                                                  float4 *__restrict__ splats)
{
    assume_model<kModel>(T);
    sp_walk(T, points, bounds, total, m, u, splats,
            [&](uint64_t p, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, float *J) {
                return trace_back_ray_jacobian_spectral(T, D, lambda[p], ox, oy, oz, dx, dy, dz, sx, sy, J);
            });
}

int launch_splat_points(const TraceBackTable &T, const float *d_points, const void *d_bounds, uint64_t n, uint32_t m, const float *d_u,
                        void *d_splats, void *stream)
{
    if (n == 0) return 0;
    if (m == 0) return static_cast<int>(hipErrorInvalidValue);
    const uint64_t total = n * m;
    const auto kernel = model_instance(T, splat_kernel<kModelThin>, splat_kernel<kModelKolb>, splat_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(total), stream, T, d_points, static_cast<const float4 *>(d_bounds), total, m,
                       reinterpret_cast<const float2 *>(d_u), static_cast<float4 *>(d_splats));
}

int launch_splat_points_spectral(const TraceBackTable &T, const BackwardDispersion &D, const float *d_points, const void *d_bounds,
                                 const float *d_lambda, uint64_t n, uint32_t m, const float *d_u, void *d_splats, void *stream)
{
    if (n == 0) return 0;
    if (m == 0) return static_cast<int>(hipErrorInvalidValue);
    const uint64_t total = n * m;
    const auto kernel = model_instance(T, splat_spectral_kernel<kModelThin>, splat_spectral_kernel<kModelKolb>, splat_spectral_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(total), stream, T, D, d_points, static_cast<const float4 *>(d_bounds), d_lambda, total, m,
                       reinterpret_cast<const float2 *>(d_u), static_cast<float4 *>(d_splats));
}

}  // namespace zoic

// traceback_jacobian.hip -- the batch trace-back with its Jacobian (traceback_jacobian.hpp): one camera ray per lane.
//
// Mapping as traceback.hip: wave64, 256-lane workgroups, a grid of at most kTbjGridCap workgroups; a larger batch is walked slab by
// slab by the same lanes.  The TraceBackTable (and, spectral, the BackwardDispersion) arrives by value as a kernel argument; the
// interface loop's index is wave-uniform, so every table entry is a scalar load.  No LDS, no scratch: the four tangents are 24
// registers.  A lane reads what the trace-back kernels read (its 32-byte record; spectral: one more dword) and writes one float2,
// if asked one flag word, and its 48 bytes of J as three 16-byte stores (a wave's 3 KiB are contiguous).
#include <hip/hip_runtime.h>

#include "traceback_jacobian.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kTbjBlock = 256;
constexpr uint64_t kTbjGridCap = 2048;

__device__ __forceinline__ void store_jacobian(float4 *__restrict__ jac, uint64_t i, const float *J)
{
    jac[3u * i] = make_float4(J[0], J[1], J[2], J[3]);
    jac[3u * i + 1u] = make_float4(J[4], J[5], J[6], J[7]);
    jac[3u * i + 2u] = make_float4(J[8], J[9], J[10], J[11]);
}

}  // namespace

// budget: 0 scratch, 0 spills, 0 LDS
__global__ __launch_bounds__(kTbjBlock) void trace_back_jacobian_kernel(const TraceBackTable T, const float4 *__restrict__ rays, uint64_t n,
                                                                        float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                                                        float4 *__restrict__ jac)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTbjBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTbjBlock + threadIdx.x; i < n; i += stride) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];   // ox oy oz dx | dy dz weight flags
        float sx, sy, J[12];
        const uint32_t f = trace_back_ray_jacobian(T, a.x, a.y, a.z, a.w, b.x, b.y, sx, sy, J);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
        store_jacobian(jac, i, J);
    }
}

// budget: 0 scratch, 0 spills, 0 LDS
__global__ __launch_bounds__(kTbjBlock) void trace_back_jacobian_spectral_kernel(const TraceBackTable T, const BackwardDispersion D,
                                                                                 const float4 *__restrict__ rays,
                                                                                 const float *__restrict__ lambda, uint64_t n,
                                                                                 float2 *__restrict__ screen, uint32_t *__restrict__ flags,
                                                                                 float4 *__restrict__ jac)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTbjBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTbjBlock + threadIdx.x; i < n; i += stride) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];
        float sx, sy, J[12];
        const uint32_t f = trace_back_ray_jacobian_spectral(T, D, lambda[i], a.x, a.y, a.z, a.w, b.x, b.y, sx, sy, J);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
        store_jacobian(jac, i, J);
    }
}

int launch_trace_back_jacobian(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian,
                               void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kTbjBlock - 1) / kTbjBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kTbjGridCap ? blocks : kTbjGridCap));
    hipLaunchKernelGGL(trace_back_jacobian_kernel, grid, dim3(kTbjBlock), 0, static_cast<hipStream_t>(stream), T,
                       static_cast<const float4 *>(d_rays), n, reinterpret_cast<float2 *>(d_screen), d_flags,
                       reinterpret_cast<float4 *>(d_jacobian));
    return static_cast<int>(hipGetLastError());
}

int launch_trace_back_jacobian_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda,
                                        uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian, void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kTbjBlock - 1) / kTbjBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kTbjGridCap ? blocks : kTbjGridCap));
    hipLaunchKernelGGL(trace_back_jacobian_spectral_kernel, grid, dim3(kTbjBlock), 0, static_cast<hipStream_t>(stream), T, D,
                       static_cast<const float4 *>(d_rays), d_lambda, n, reinterpret_cast<float2 *>(d_screen), d_flags,
                       reinterpret_cast<float4 *>(d_jacobian));
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

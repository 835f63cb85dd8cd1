// traceback_spectral.hip -- the batch trace-back at a wavelength per ray (backward_spectral.hpp): one camera ray per lane.
//
// Mapping as traceback.hip: wave64, 256-lane workgroups, a grid of at most kTbsGridCap workgroups striding the batch.  The
// TraceBackTable and the BackwardDispersion arrive by value as kernel arguments; the interface loop's index is wave-uniform, so an
// interface is one 16-byte and one 8-byte scalar load.  A lane reads its 32-byte record and one more coalesced dword, its
// wavelength (48 bytes per ray moved against 44), computes dl once, and per interface one index (a multiply and an add) and one
// division on top of the d-line trace.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "backward_spectral.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kTbsBlock = 256;
constexpr uint64_t kTbsGridCap = 2048;

}  // namespace

// budget: 0 scratch, 0 spills, 0 LDS, at most 64 VGPRs (8 waves per SIMD)
__global__ __launch_bounds__(kTbsBlock) void trace_back_spectral_kernel(const TraceBackTable T, const BackwardDispersion D,
                                                                        const float4 *__restrict__ rays, const float *__restrict__ lambda,
                                                                        uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTbsBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTbsBlock + threadIdx.x; i < n; i += stride) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];   // ox oy oz dx | dy dz weight flags
        float sx, sy;
        const uint32_t f = trace_back_ray_spectral(T, D, lambda[i], a.x, a.y, a.z, a.w, b.x, b.y, sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    }
}

int launch_trace_back_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda, uint64_t n,
                               float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kTbsBlock - 1) / kTbsBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kTbsGridCap ? blocks : kTbsGridCap));
    hipLaunchKernelGGL(trace_back_spectral_kernel, grid, dim3(kTbsBlock), 0, static_cast<hipStream_t>(stream), T, D,
                       static_cast<const float4 *>(d_rays), d_lambda, n, reinterpret_cast<float2 *>(d_screen), d_flags);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

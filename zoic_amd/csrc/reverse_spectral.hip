// reverse_spectral.hip -- the batch reverse projection at a wavelength per point (backward_spectral.hpp): one point per lane.
//
// Mapping as reverse.hip: wave64, 256-lane workgroups, a grid of at most kRevsGridCap workgroups striding the batch.  The
// ReverseTable and the BackwardDispersion arrive by value as kernel arguments; the interface loops' index is wave-uniform, so every
// table read is a scalar load (the dispersion entry: one 8-byte load).  A lane reads its packed float3 and one more coalesced
// dword, its wavelength, computes dl and the index in front of the stop once, and in every pass of the search one index and one
// division per interface on top of the d-line pass.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "backward_spectral.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kRevsBlock = 256;
constexpr uint64_t kRevsGridCap = 2048;

}  // namespace

// budget: 0 scratch, 0 spills, at most 64 VGPRs (8 waves per SIMD)
__global__ __launch_bounds__(kRevsBlock) void project_points_spectral_kernel(const ReverseTable T, const BackwardDispersion D,
                                                                             const float *__restrict__ points, const float *__restrict__ lambda,
                                                                             uint64_t n, float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kRevsBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kRevsBlock + threadIdx.x; i < n; i += stride) {
        const float *p = points + i * 3u;
        float sx, sy;
        const uint32_t f = project_point_spectral(T, D, lambda[i], p[0], p[1], p[2], sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    }
}

int launch_project_points_spectral(const ReverseTable &T, const BackwardDispersion &D, const float *d_points, const float *d_lambda,
                                   uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kRevsBlock - 1) / kRevsBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kRevsGridCap ? blocks : kRevsGridCap));
    hipLaunchKernelGGL(project_points_spectral_kernel, grid, dim3(kRevsBlock), 0, static_cast<hipStream_t>(stream), T, D, d_points, d_lambda,
                       n, reinterpret_cast<float2 *>(d_screen), d_flags);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

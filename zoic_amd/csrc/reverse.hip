// reverse.hip -- the batch reverse projection (reverse.hpp): one point per lane.
//
// Mapping: wave64, 256-lane workgroups, a grid of at most kRevGridCap workgroups; a batch larger than one grid's worth (a slab of
// kRevGridCap x 256 points) is walked slab by slab by the same lanes.  The ReverseTable arrives by value as a kernel argument: the
// interface loop's index is wave-uniform, so every table read is a scalar load.  No LDS, no scratch.  A lane reads its packed
// float3 (three dword loads; a wave's 768 bytes are contiguous), runs the search of project_point -- the lanes of a wave loop
// until the last of them has converged -- and writes one float2 and, if asked, one flag word.
#include <hip/hip_runtime.h>

#include "reverse.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kRevBlock = 256;
constexpr uint64_t kRevGridCap = 2048;

}  // namespace

// budget: 0 scratch, 0 spills
__global__ __launch_bounds__(kRevBlock) void project_points_kernel(const ReverseTable T, const float *__restrict__ points, uint64_t n,
                                                                   float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kRevBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kRevBlock + threadIdx.x; i < n; i += stride) {
        const float *p = points + i * 3u;
        float sx, sy;
        const uint32_t f = project_point(T, p[0], p[1], p[2], sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    }
}

int launch_project_points(const ReverseTable &T, const float *d_points, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kRevBlock - 1) / kRevBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kRevGridCap ? blocks : kRevGridCap));
    hipLaunchKernelGGL(project_points_kernel, grid, dim3(kRevBlock), 0, static_cast<hipStream_t>(stream), T, d_points, n,
                       reinterpret_cast<float2 *>(d_screen), d_flags);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

// traceback.hip -- the batch trace-back (traceback.hpp): one camera ray per lane.
//
// Mapping: wave64, 256-lane workgroups, a grid of at most kTbGridCap workgroups; a batch larger than one grid's worth (a slab of
// kTbGridCap x 256 rays) is walked slab by slab by the same lanes.  The TraceBackTable arrives by value as a kernel argument: the
// interface loop's index is wave-uniform, so every table entry is one 16-byte scalar load.  No LDS, no scratch.  A lane reads its 32-byte
// record as two 16-byte loads (a wave's 2 KiB are contiguous; the compiler narrows the second to the 8 bytes that are used), runs
// trace_back_ray -- one pass over the interfaces, a lane whose ray has ended waits for the wave's loop -- and writes one float2 and,
// if asked, one flag word.
#include <hip/hip_runtime.h>

#include "traceback.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kTbBlock = 256;
constexpr uint64_t kTbGridCap = 2048;

}  // namespace

// budget: 0 scratch, 0 spills, 0 LDS
__global__ __launch_bounds__(kTbBlock) void trace_back_kernel(const TraceBackTable T, const float4 *__restrict__ rays, uint64_t n,
                                                              float2 *__restrict__ screen, uint32_t *__restrict__ flags)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTbBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTbBlock + threadIdx.x; i < n; i += stride) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];   // ox oy oz dx | dy dz weight flags
        float sx, sy;
        const uint32_t f = trace_back_ray(T, a.x, a.y, a.z, a.w, b.x, b.y, sx, sy);
        screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    }
}

int launch_trace_back(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream)
{
    if (n == 0) return 0;
    const uint64_t blocks = (n + kTbBlock - 1) / kTbBlock;
    const dim3 grid(static_cast<uint32_t>(blocks < kTbGridCap ? blocks : kTbGridCap));
    hipLaunchKernelGGL(trace_back_kernel, grid, dim3(kTbBlock), 0, static_cast<hipStream_t>(stream), T, static_cast<const float4 *>(d_rays), n,
                       reinterpret_cast<float2 *>(d_screen), d_flags);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

// device_pass.hpp -- the shape every opt-in pass shares (differentials, spectral and hero rays, transmittance, ghosts, reverse projection,
// trace-back, pupil bounds, splats): the launch shape, the one-item-per-lane walk, the typed view of a kernel's own arguments and the
// launchers' tail.
//
// Mapping: wave64, kPassBlock = 256 lanes per workgroup, a grid of at most kPassGridCap = 2048 workgroups (8 waves per SIMD on 256 CUs);
// a batch larger than one grid's worth (a slab of kPassGridCap x kPassBlock items) is walked slab by slab by the same lanes, with a
// 64-bit index.  What an item is -- a ray, a sample, a wave's point, a wave's chunk -- is the kernel's own: it says so by the
// itemsPerBlock it gives pass_grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace zoic {

constexpr int kPassBlock = 256;
constexpr uint64_t kPassGridCap = 2048;

inline dim3 pass_grid(uint64_t items, uint64_t itemsPerBlock = kPassBlock)
{
    const uint64_t blocks = (items + itemsPerBlock - 1) / itemsPerBlock;
    return dim3(static_cast<uint32_t>(blocks < kPassGridCap ? blocks : kPassGridCap));
}

// the grid's stride, in lanes
static __device__ __forceinline__ uint64_t pass_stride() { return static_cast<uint64_t>(gridDim.x) * kPassBlock; }

// one item per lane: body(i) for the lane's items i < n, a grid stride apart
template <class Body>
static __device__ __forceinline__ void for_each_item(uint64_t n, Body body)
{
    const uint64_t stride = pass_stride();
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPassBlock + threadIdx.x; i < n; i += stride) body(i);
}

// A kernel that reads a by-value table with scalar loads at a wave-uniform index restates its parameter list as a struct (HIP lays
// kernel arguments out like a C struct, kolb_pool_body.hpp KolbKernelArgs) and takes a typed pointer into the kernel-argument segment at
// offsetof(that struct, field).  Kernel arguments are limited to 4 KB, the 256 bytes of hidden arguments the compiler appends included.
template <class T>
using KernargPtr = const T __attribute__((address_space(4))) *;

template <class KernelArgs, class T>
static __device__ __forceinline__ KernargPtr<T> kernarg_view(size_t offset)
{
    static_assert(sizeof(KernelArgs) + 256 <= 4096, "the kernel's arguments no longer fit in 4 KB: a table has to stay in device memory");
    return (KernargPtr<T>)((KernargPtr<char>)__builtin_amdgcn_kernarg_segment_ptr() + offset);
}

// the launchers' tail: kPassBlock lanes, no dynamic LDS, the caller's stream; the launch's error code
template <class Kernel, class... Args>
inline int launch_pass(Kernel kernel, dim3 grid, void *stream, const Args &...args)
{
    hipLaunchKernelGGL(kernel, grid, dim3(kPassBlock), 0, static_cast<hipStream_t>(stream), args...);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

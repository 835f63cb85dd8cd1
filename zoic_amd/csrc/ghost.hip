// ghost.hip -- ghost rays (ghost.hpp): one pass over records that already exist, those of zoic_create_rays_device or
// zoic_create_rays_spectral_device, that writes p ghost records per sample.
//
// Mapping as the transmittance pass (transmittance.hip): one SAMPLE per lane, wave64, 256-lane workgroups, a grid of at most 2048
// workgroups striding over the batch a wave (64 consecutive samples) at a time.  A lane first reads the weight and the flags of its
// main record and, where it has weight, its wavelength.  A wave without a live lane writes its dead records and never reads a sample.
// Otherwise the accepted try is replayed ONCE per sample (kolb_replay) and the p pairs are a wave-uniform loop around that start.
// Within one pair the whole interface sequence (leg, index, refract or reflect) is wave-uniform, so every table entry is a scalar load
// at a readfirstlane'd index: the dispersion, the films and the pairs through the kernel-argument segment (spectral.hpp ZOIC_SPEC_PIN),
// the geometry from the camera's GhostTable in device memory -- the kernel arguments have no room for it beside the KolbTable that the
// replay takes (the static_assert below).  Records leave as whole 32-byte stores, sample-major, n x p.  Nothing goes to scratch.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "differentials_device.hpp"
#include "ghost.hpp"
#include "ray_store.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

struct GhostPairs { uint32_t packed[kGhostMaxPairs]; };   // a | b << 8, by value: the call needs no staging buffer

// The kernel's argument list as a struct (HIP lays kernel arguments out like a C struct, kolb_pool_body.hpp KolbKernelArgs)
struct GhostKernelArgs {
    KolbTable T; GhostMedia M; BokehTables B; GhostPairs P; const GhostTable *G; const float4 *samples; const float *lambdas; const uint4 *rngStates;
    uint64_t rayBase; uint64_t n; const RayRecord *rays; RayRecord *out; uint32_t p;
};
// kernel arguments are limited to 4 KB, the 256 bytes of hidden arguments the compiler appends included
static_assert(sizeof(GhostKernelArgs) + 256 <= 4096, "the ghost kernel's arguments no longer fit: the geometry stays in device memory");

typedef const char __attribute__((address_space(4))) *KernargBytes;
typedef const GhostMedia __attribute__((address_space(4))) *GhostMediaPtr;
typedef const uint32_t __attribute__((address_space(4))) *GhostPairsPtr;
__device__ __forceinline__ GhostMediaPtr kernarg_media()
{
    return (GhostMediaPtr)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(GhostKernelArgs, M));
}
__device__ __forceinline__ GhostPairsPtr kernarg_pairs()
{
    return (GhostPairsPtr)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(GhostKernelArgs, P));
}

constexpr float kLambdaD32 = 587.5618f;   // d_lambda == nullptr: the d-line (spectral_dl gives exactly 0 there)

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_ghost_kernel(
    const KolbTable T, const GhostMedia M, const BokehTables B, const GhostPairs P, const GhostTable *__restrict__ G,
    const float4 *__restrict__ samples, const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n,
    const RayRecord *__restrict__ rays, RayRecord *__restrict__ out, uint32_t p)
{
    __shared__ __align__(16) float2 lut[kLutEntries];   // (maxScale, centroid.x) pairs of the exit-pupil LUT: setup_ray's lookup
    if (threadIdx.x < kLutEntries) lut[threadIdx.x] = make_float2(T.lutMaxScale[threadIdx.x], T.lutCentroidX[threadIdx.x]);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + wave * 64u; base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        const float4 r1 = reinterpret_cast<const float4 *>(rays + (have ? i : base))[1];   // dy dz weight flags
        const bool start = have && r1.z != 0.0f;
        float lambda = kLambdaD32;
        if (start && lambdas) lambda = lambdas[i];   // a lane without a start reads no wavelength
        const bool live = start && spectral_valid(lambda);
        V3 o0{0.f, 0.f, 0.f}, d0{0.f, 0.f, 0.f};
        if (__ballot(live) != 0ull && live) {
            const uint32_t tries = (__builtin_bit_cast(uint32_t, r1.w) >> 1) & 31u;
            kolb_replay(T, B, lut, samples[i], tries, rngStates, rayBase, i, [&](V3 o, V3 d) { o0 = o; d0 = d; return 0; });
        }
        for (uint32_t jj = 0; jj < p; ++jj) {
            const uint32_t j = __builtin_amdgcn_readfirstlane(jj);
            GhostPairsPtr pairs = kernarg_pairs();
            ZOIC_SPEC_PIN(pairs);
            const uint32_t pair = pairs[j];
            const GhostRay g = ghost_record(G, kernarg_media(), pair, start, lambda, o0, d0);
            if (have) store_ray_record(out, i * p + j, g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.weight, g.flags);
        }
    }
}

// THINLENS / NONE: a lens without interfaces has no ghosts.  One record per lane.
__global__ __launch_bounds__(kDiffBlock) void ghost_model_kernel(uint64_t total, RayRecord *__restrict__ out)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + threadIdx.x; e < total; e += stride)
        store_ray_record(out, e, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, kGhostModel << kGhostReasonShift);
}

int launch_ghost_rays(int model, const KolbTable &kolb, const GhostMedia &media, const BokehTables &bokeh, const GhostTable *d_table,
                      uint32_t p, const uint32_t *pairs, const float *d_samples, const float *d_lambda, const uint32_t *d_rng,
                      uint64_t rayBase, uint64_t n, const RayRecord *rays, RayRecord *d_out, void *stream)
{
    if (n == 0) return 0;
    if (p == 0 || p > static_cast<uint32_t>(kGhostMaxPairs)) return static_cast<int>(hipErrorInvalidValue);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (model == 1) {
        if (!d_table) return static_cast<int>(hipErrorInvalidValue);
        GhostPairs P{};
        for (uint32_t j = 0; j < p; ++j) P.packed[j] = pairs[j];
        hipLaunchKernelGGL(kolb_ghost_kernel, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, kolb, media, bokeh, P, d_table,
                           reinterpret_cast<const float4 *>(d_samples), d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, p);
    } else {
        hipLaunchKernelGGL(ghost_model_kernel, dim3(diff_grid(n * p)), dim3(kDiffBlock), 0, s, n * p, d_out);
    }
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

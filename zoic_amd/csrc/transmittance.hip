// transmittance.hip -- the Fresnel transmittance of traced rays (transmittance.hpp): one pass over records that already exist, those of
// zoic_create_rays_device, zoic_create_rays_spectral_device (k == 1) or zoic_create_rays_hero_device (k >= 2).
//
// Mapping as the differential kernels (differentials_device.hpp): one SAMPLE per lane, wave64, 256-lane workgroups, a grid of at most
// 2048 workgroups striding over the batch a wave (64 consecutive samples) at a time.  A lane first reads the weights of its k records and
// the wavelengths of those that have one: a column is live where the weight is not 0 and the wavelength is valid.  A wave without a live
// column writes zeros and never reads a sample.  Otherwise the accepted try is replayed ONCE per sample (kolb_replay with column 0's try
// count: the hero's start is every companion's) and the k columns are a wave-uniform loop around it, each live column one primal trace
// at its own wavelength with the observer of transmittance.hpp riding along.  The interfaces, the dispersion table and the film table
// arrive by value and are read through the kernel-argument segment (spectral.hpp ZOIC_SPEC_PIN) with scalar loads at the wave-uniform
// interface index.  The n x k floats leave as coalesced stores: directly for k == 1, through a per-wave LDS transpose otherwise.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "differentials_device.hpp"
#include "hero.hpp"
#include "transmittance.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// The Kolb kernel's argument list as a struct (HIP lays kernel arguments out like a C struct, kolb_pool_body.hpp KolbKernelArgs)
struct TransmittanceKernelArgs {
    KolbTable T; SpectralTable W; FilmTable F; BokehTables B; const float4 *samples; const float *lambdas; const uint4 *rngStates;
    uint64_t rayBase; uint64_t n; const RayRecord *rays; float *out; uint32_t k;
};
// kernel arguments are limited to 4 KB, the 256 bytes of hidden arguments the compiler appends included
static_assert(sizeof(TransmittanceKernelArgs) + 256 <= 4096, "the film table no longer fits beside the other tables: pass a KolbTable without fsurf");

typedef const char __attribute__((address_space(4))) *KernargBytes;
typedef const Surface __attribute__((address_space(4))) *SurfaceTable;
typedef const SpectralTable __attribute__((address_space(4))) *SpectralTablePtr;
typedef const FilmTable __attribute__((address_space(4))) *FilmTablePtr;
__device__ __forceinline__ SurfaceTable kernarg_surfaces()
{
    return (SurfaceTable)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TransmittanceKernelArgs, T) + offsetof(KolbTable, surf));
}
__device__ __forceinline__ SpectralTablePtr kernarg_spectral()
{
    return (SpectralTablePtr)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TransmittanceKernelArgs, W));
}
__device__ __forceinline__ FilmTablePtr kernarg_film()
{
    return (FilmTablePtr)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TransmittanceKernelArgs, F));
}

constexpr float kLambdaD32 = 587.5618f;   // d_lambda == nullptr: the d-line (spectral_dl gives exactly 0 there)

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_transmittance_kernel(
    const KolbTable T, const SpectralTable W, const FilmTable F, const BokehTables B, const float4 *__restrict__ samples,
    const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays,
    float *__restrict__ out, uint32_t k)
{
    __shared__ __align__(16) float2 lut[kLutEntries];   // (maxScale, centroid.x) pairs of the exit-pupil LUT: setup_ray's lookup
    __shared__ float stage[kDiffBlock / 64][64 * kHeroMaxWavelengths];
    if (threadIdx.x < kLutEntries) lut[threadIdx.x] = make_float2(T.lutMaxScale[threadIdx.x], T.lutCentroidX[threadIdx.x]);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *st = stage[wave];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + wave * 64u; base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        const uint64_t row = (have ? i : base) * k;     // (a lane past the end reads the wave's first row and writes nothing)
        uint32_t liveColumns = 0;                       // bit j: record (i, j) has weight and a valid wavelength
        for (uint32_t j = 0; j < k; ++j) {
            bool live = have && rays[row + j].weight != 0.0f;
            if (live && lambdas) live = spectral_valid(lambdas[row + j]);   // a dead column reads no wavelength
            liveColumns |= (live ? 1u : 0u) << j;
        }
        const bool any = liveColumns != 0u;
        V3 o0{0.f, 0.f, 0.f}, d0{0.f, 0.f, 0.f};
        if (__ballot(any) != 0ull && any) {
            const uint32_t tries = (rays[row].flags >> 1) & 31u;   // column 0's: the hero's accepted try
            kolb_replay(T, B, lut, samples[i], tries, rngStates, rayBase, i, [&](V3 o, V3 d) { o0 = o; d0 = d; return 0; });
        }
        for (uint32_t jj = 0; jj < k; ++jj) {
            const uint32_t j = __builtin_amdgcn_readfirstlane(jj);
            const bool live = ((liveColumns >> j) & 1u) != 0u;
            float t = 0.0f;
            if (__ballot(live) != 0ull && live) {
                const float lambda = lambdas ? lambdas[row + j] : kLambdaD32;
                t = path_transmittance(kernarg_surfaces(), kernarg_spectral(), kernarg_film(), T.lensCount, lambda, o0, d0);
            }
            if (k == 1u) { if (have) out[i] = t; }
            else st[lane * k + j] = t;
        }
        if (k > 1u) {
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes have landed
            const uint64_t left = n - base;
            const uint32_t valid = (left < 64u ? static_cast<uint32_t>(left) : 64u) * k;
            float *dst = out + base * k;
            for (uint32_t m = 0; m < k; ++m) {
                const uint32_t e = m * 64u + lane;
                if (e < valid) dst[e] = st[e];
            }
            __builtin_amdgcn_wave_barrier();   // the next wave-tile overwrites the stage
        }
    }
}

// THINLENS: a thin lens has no interface; 1.0 where the record has weight and the wavelength is valid.  One record per lane.
__global__ __launch_bounds__(kDiffBlock) void thin_transmittance_kernel(const float *__restrict__ lambdas, const RayRecord *__restrict__ rays,
                                                                        uint64_t total, float *__restrict__ out)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + threadIdx.x; e < total; e += stride) {
        bool live = rays[e].weight != 0.0f;
        if (live && lambdas) live = spectral_valid(lambdas[e]);
        out[e] = live ? 1.0f : 0.0f;
    }
}

int launch_ray_transmittance(int model, const KolbTable &kolb, const SpectralTable &spec, const FilmTable &film, const BokehTables &bokeh,
                             const float *d_samples, const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k,
                             const RayRecord *rays, float *d_out, void *stream)
{
    if (n == 0) return 0;
    if (k == 0 || k > kHeroMaxWavelengths) return static_cast<int>(hipErrorInvalidValue);   // the stage holds 64 x kHeroMaxWavelengths floats
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (model == 1)
        hipLaunchKernelGGL(kolb_transmittance_kernel, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, kolb, spec, film, bokeh,
                           reinterpret_cast<const float4 *>(d_samples), d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, k);
    else
        hipLaunchKernelGGL(thin_transmittance_kernel, dim3(diff_grid(n * k)), dim3(kDiffBlock), 0, s, d_lambda, rays, n * k, d_out);
    return static_cast<int>(hipGetLastError());
}

}  // namespace zoic

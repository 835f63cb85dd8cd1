// transmittance.hip -- the Fresnel transmittance of traced rays (transmittance.hpp): one pass over records that already exist, those of
// zoic_create_rays_device, zoic_create_rays_spectral_device (k == 1) or zoic_create_rays_hero_device (k >= 2).
//
// Mapping: one SAMPLE per lane, the record pass of record_pass.hpp (launch shape: device_pass.hpp).  A lane first reads the weights of
// its k records and the wavelengths of those that have one: a column is live where the weight is not 0 and the wavelength is valid.  A
// wave without a live column writes zeros and never reads a sample.  Otherwise the accepted try is replayed ONCE per sample
// (accepted_start with column 0's try count: the hero's start is every companion's) and the k columns are a wave-uniform loop around it,
// each live column one primal trace at its own wavelength with the observer of transmittance.hpp riding along.  The interfaces, the
// dispersion table and the film table arrive by value and are read through the kernel-argument segment (device_pass.hpp kernarg_view,
// spectral.hpp ZOIC_SPEC_PIN) with scalar loads at the wave-uniform interface index.  The n x k floats leave as coalesced stores:
// directly for k == 1, through the wave's stage otherwise.
// Multilayer coatings (coating_stack.hpp): a camera with a stack on any interface runs kolb_stack_loss_kernel, the same body under the
// coating policy `const StackTable *` -- the camera's table in device memory, read with scalar loads at the same wave-uniform index.
// A camera without stacks runs kolb_transmittance_kernel as before.
#include <hip/hip_runtime.h>

#include "coating_stack.hpp"
#include "hero.hpp"
#include "record_pass.hpp"
#include "transmittance.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// the Kolb kernel's argument list (device_pass.hpp kernarg_view: were the film table not to fit beside the others, pass a KolbTable without fsurf)
struct TransmittanceKernelArgs {
    KolbTable T; SpectralTable W; FilmTable F; BokehTables B; const float4 *samples; const float *lambdas; const uint4 *rngStates;
    uint64_t rayBase; uint64_t n; const RayRecord *rays; float *out; uint32_t k;
};
__device__ __forceinline__ auto kernarg_surfaces()
{
    return kernarg_view<TransmittanceKernelArgs, Surface>(offsetof(TransmittanceKernelArgs, T) + offsetof(KolbTable, surf));
}
__device__ __forceinline__ auto kernarg_spectral() { return kernarg_view<TransmittanceKernelArgs, SpectralTable>(offsetof(TransmittanceKernelArgs, W)); }
__device__ __forceinline__ auto kernarg_film() { return kernarg_view<TransmittanceKernelArgs, FilmTable>(offsetof(TransmittanceKernelArgs, F)); }

// the one body of both Kolb kernels; KP: the coating policy.  (The stack-aware kernel's extra argument comes last: the offsets of
// TransmittanceKernelArgs hold for both.)
template <class KP>
__device__ __forceinline__ void transmittance_pass(const KolbTable &T, const BokehTables &B, const float4 *__restrict__ samples,
                                                   const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase,
                                                   uint64_t n, const RayRecord *__restrict__ rays, float *__restrict__ out, uint32_t k, KP K)
{
    __shared__ __align__(16) float2 lut[kLutEntries];
    __shared__ float stage[kPassBlock / 64][64 * kHeroMaxWavelengths];
    stage_lut(T, lut);
    float *st = stage[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = pass_stride();
    for (uint64_t base = first_wave_tile(); base < n; base += stride) {
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
        if (__ballot(any) != 0ull && any)   // column 0's tries: the hero's accepted try
            accepted_start(T, B, lut, samples[i], record_tries(rays[row].flags), rngStates, rayBase, i, o0, d0);
        for (uint32_t jj = 0; jj < k; ++jj) {
            const uint32_t j = __builtin_amdgcn_readfirstlane(jj);
            const bool live = ((liveColumns >> j) & 1u) != 0u;
            float t = 0.0f;
            if (__ballot(live) != 0ull && live) {
                const float lambda = lambdas ? lambdas[row + j] : kLambdaD32;   // d_lambda == nullptr: the d-line
                t = path_transmittance(kernarg_surfaces(), kernarg_spectral(), kernarg_film(), K, T.lensCount, lambda, o0, d0);
            }
            if (k == 1u) { if (have) out[i] = t; }
            else st[lane * k + j] = t;
        }
        if (k > 1u) staged_store(st, out + base * k, tile_valid(n, base), k);
    }
}

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_transmittance_kernel(
    const KolbTable T, const SpectralTable W, const FilmTable F, const BokehTables B, const float4 *__restrict__ samples,
    const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays,
    float *__restrict__ out, uint32_t k)
{
    transmittance_pass(T, B, samples, lambdas, rngStates, rayBase, n, rays, out, k, NoStacks{});
}

// the same with multilayer coatings; budget: the plain kernel's, and no LDS beyond its
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_stack_loss_kernel(
    const KolbTable T, const SpectralTable W, const FilmTable F, const BokehTables B, const float4 *__restrict__ samples,
    const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays,
    float *__restrict__ out, uint32_t k, const StackTable *__restrict__ stacks)
{
    transmittance_pass(T, B, samples, lambdas, rngStates, rayBase, n, rays, out, k, stacks);
}

// THINLENS: a thin lens has no interface; 1.0 where the record has weight and the wavelength is valid.  One record per lane.
__global__ __launch_bounds__(kPassBlock) void thin_transmittance_kernel(const float *__restrict__ lambdas, const RayRecord *__restrict__ rays,
                                                                        uint64_t total, float *__restrict__ out)
{
    for_each_item(total, [&](uint64_t e) {
        bool live = rays[e].weight != 0.0f;
        if (live && lambdas) live = spectral_valid(lambdas[e]);
        out[e] = live ? 1.0f : 0.0f;
    });
}

int launch_ray_transmittance(int model, const KolbTable &kolb, const SpectralTable &spec, const FilmTable &film, const BokehTables &bokeh,
                             const float *d_samples, const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k,
                             const RayRecord *rays, float *d_out, void *stream, const StackTable *d_stacks)
{
    if (n == 0) return 0;
    if (k == 0 || k > kHeroMaxWavelengths) return static_cast<int>(hipErrorInvalidValue);   // the stage holds 64 x kHeroMaxWavelengths floats
    if (model == 1 && d_stacks)
        return launch_pass(kolb_stack_loss_kernel, pass_grid(n), stream, kolb, spec, film, bokeh, reinterpret_cast<const float4 *>(d_samples),
                           d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, k, d_stacks);
    if (model == 1)
        return launch_pass(kolb_transmittance_kernel, pass_grid(n), stream, kolb, spec, film, bokeh, reinterpret_cast<const float4 *>(d_samples),
                           d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, k);
    return launch_pass(thin_transmittance_kernel, pass_grid(n * k), stream, d_lambda, rays, n * k, d_out);
}

}  // namespace zoic

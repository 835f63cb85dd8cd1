// ghost.hip -- ghost rays (ghost.hpp): one pass over records that already exist, those of zoic_create_rays_device or
// zoic_create_rays_spectral_device, that writes p ghost records per sample.
//
// Mapping: one SAMPLE per lane, the record pass of record_pass.hpp (launch shape: device_pass.hpp).  A lane first reads the weight and
// the flags of its main record and, where it has weight, its wavelength.  A wave without a live lane writes its dead records and never
// reads a sample.  Otherwise the accepted try is replayed ONCE per sample (accepted_start) and the p pairs are a wave-uniform loop around
// that start.  Within one pair the whole interface sequence (leg, index, refract or reflect) is wave-uniform, so every table entry is a
// scalar load at a readfirstlane'd index: the dispersion, the films and the pairs through the kernel-argument segment (device_pass.hpp
// kernarg_view, spectral.hpp ZOIC_SPEC_PIN), the geometry from the camera's GhostTable in device memory -- the kernel arguments have no
// room for it beside the KolbTable that the replay takes.  Records leave as whole 32-byte stores, sample-major, n x p: no stage.  Nothing
// goes to scratch.
// Multilayer coatings (coating_stack.hpp): a camera with a stack on any interface runs kolb_stack_flare_kernel, the same body under the
// coating policy `const StackTable *` -- the camera's table in device memory beside its GhostTable, scalar loads at the same index.
#include <hip/hip_runtime.h>

#include "ghost.hpp"
#include "ray_store.hpp"
#include "record_pass.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

struct GhostPairs { uint32_t packed[kGhostMaxPairs]; };   // a | b << 8, by value: the call needs no staging buffer

// the kernel's argument list (device_pass.hpp kernarg_view)
struct GhostKernelArgs {
    KolbTable T; GhostMedia M; BokehTables B; GhostPairs P; const GhostTable *G; const float4 *samples; const float *lambdas; const uint4 *rngStates;
    uint64_t rayBase; uint64_t n; const RayRecord *rays; RayRecord *out; uint32_t p;
};
__device__ __forceinline__ auto kernarg_media() { return kernarg_view<GhostKernelArgs, GhostMedia>(offsetof(GhostKernelArgs, M)); }
__device__ __forceinline__ auto kernarg_pairs() { return kernarg_view<GhostKernelArgs, uint32_t>(offsetof(GhostKernelArgs, P)); }

// the one body of both Kolb kernels; KP: the coating policy.  (The stack-aware kernel's extra argument comes last: the offsets of
// GhostKernelArgs hold for both.)
template <class KP>
__device__ __forceinline__ void ghost_pass(const KolbTable T, const BokehTables B, const GhostTable *__restrict__ G,
                                           const float4 *__restrict__ samples, const float *__restrict__ lambdas,
                                           const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n,
                                           const RayRecord *__restrict__ rays, RayRecord *__restrict__ out, uint32_t p, KP K)
{
    __shared__ __align__(16) float2 lut[kLutEntries];
    stage_lut(T, lut);
    const uint64_t stride = pass_stride();
    for (uint64_t base = first_wave_tile(); base < n; base += stride) {
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool have = i < n;
        const float4 r1 = reinterpret_cast<const float4 *>(rays + (have ? i : base))[1];   // dy dz weight flags
        const bool start = have && r1.z != 0.0f;
        float lambda = kLambdaD32;                   // d_lambda == nullptr: the d-line
        if (start && lambdas) lambda = lambdas[i];   // a lane without a start reads no wavelength
        const bool live = start && spectral_valid(lambda);
        V3 o0{0.f, 0.f, 0.f}, d0{0.f, 0.f, 0.f};
        if (__ballot(live) != 0ull && live)
            accepted_start(T, B, lut, samples[i], record_tries(__builtin_bit_cast(uint32_t, r1.w)), rngStates, rayBase, i, o0, d0);
        for (uint32_t jj = 0; jj < p; ++jj) {
            const uint32_t j = __builtin_amdgcn_readfirstlane(jj);
            auto pairs = kernarg_pairs();
            ZOIC_SPEC_PIN(pairs);
            const uint32_t pair = pairs[j];
            const GhostRay g = ghost_record(G, kernarg_media(), pair, start, lambda, o0, d0, K);
            if (have) store_ray_record(out, i * p + j, g.ox, g.oy, g.oz, g.dx, g.dy, g.dz, g.weight, g.flags);
        }
    }
}

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_ghost_kernel(
    const KolbTable T, const GhostMedia M, const BokehTables B, const GhostPairs P, const GhostTable *__restrict__ G,
    const float4 *__restrict__ samples, const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n,
    const RayRecord *__restrict__ rays, RayRecord *__restrict__ out, uint32_t p)
{
    ghost_pass(T, B, G, samples, lambdas, rngStates, rayBase, n, rays, out, p, NoStacks{});
}

// the same with multilayer coatings; budget: the plain kernel's, and no LDS beyond its
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_stack_flare_kernel(
    const KolbTable T, const GhostMedia M, const BokehTables B, const GhostPairs P, const GhostTable *__restrict__ G,
    const float4 *__restrict__ samples, const float *__restrict__ lambdas, const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n,
    const RayRecord *__restrict__ rays, RayRecord *__restrict__ out, uint32_t p, const StackTable *__restrict__ stacks)
{
    ghost_pass(T, B, G, samples, lambdas, rngStates, rayBase, n, rays, out, p, stacks);
}

// THINLENS / NONE: a lens without interfaces has no ghosts.  One record per lane.
__global__ __launch_bounds__(kPassBlock) void ghost_model_kernel(uint64_t total, RayRecord *__restrict__ out)
{
    for_each_item(total, [&](uint64_t e) { store_ray_record(out, e, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, kGhostModel << kGhostReasonShift); });
}

int launch_ghost_rays(int model, const KolbTable &kolb, const GhostMedia &media, const BokehTables &bokeh, const GhostTable *d_table,
                      uint32_t p, const uint32_t *pairs, const float *d_samples, const float *d_lambda, const uint32_t *d_rng,
                      uint64_t rayBase, uint64_t n, const RayRecord *rays, RayRecord *d_out, void *stream, const StackTable *d_stacks)
{
    if (n == 0) return 0;
    if (p == 0 || p > static_cast<uint32_t>(kGhostMaxPairs)) return static_cast<int>(hipErrorInvalidValue);
    if (model != 1) return launch_pass(ghost_model_kernel, pass_grid(n * p), stream, n * p, d_out);
    if (!d_table) return static_cast<int>(hipErrorInvalidValue);
    GhostPairs P{};
    for (uint32_t j = 0; j < p; ++j) P.packed[j] = pairs[j];
    if (d_stacks)
        return launch_pass(kolb_stack_flare_kernel, pass_grid(n), stream, kolb, media, bokeh, P, d_table, reinterpret_cast<const float4 *>(d_samples),
                           d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, p, d_stacks);
    return launch_pass(kolb_ghost_kernel, pass_grid(n), stream, kolb, media, bokeh, P, d_table, reinterpret_cast<const float4 *>(d_samples), d_lambda,
                       reinterpret_cast<const uint4 *>(d_rng), rayBase, n, rays, d_out, p);
}

}  // namespace zoic

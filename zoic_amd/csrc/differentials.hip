// differentials.hip -- the traced ray differentials (differentials.hpp): one pass over the records a ray launch wrote.
//
// Mapping: one ray per lane, the record pass of record_pass.hpp (launch shape: device_pass.hpp).  Tables arrive as by-value kernel
// arguments, as in the ray kernels: the interfaces are read with scalar loads at a wave-uniform index.  A wave first reads the second
// half of its 64 records (weight, flags): if every weight is 0 -- 79 % of a wide-open PETZVAL frame's rays -- it writes zeros and never
// reads a sample; otherwise only the live lanes read theirs, replay their retry stream up to the accepted try (the loop runs to the
// wave's largest try count), rebuild the lens point and trace one try with two tangents.  The 48-byte outputs of a wave leave as three
// fully coalesced 16-byte stores per lane (Arnold rows: 21 coalesced dword stores).  The pass itself is record_pass.hpp
// differentials_pass; this file holds the d-line ray functions and launchers.
#include <hip/hip_runtime.h>

#include "record_pass.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// RAYTRACED: the accepted try's start (record_pass.hpp), then one traced try with tangents
__device__ __forceinline__ RayDifferential kolb_ray(const KolbTable &T, const BokehTables &B, const float2 *lut, float4 s, uint32_t a,
                                                    const uint4 *rngStates, uint64_t rayBase, uint64_t i)
{
    const auto surfAt = [&](int k) { return T.surf[__builtin_amdgcn_readfirstlane(k)]; };   // wave-uniform: scalar loads
    return kolb_replay(T, B, lut, s, a, rngStates, rayBase, i, [&](V3 o0, V3 d) { return kolb_differentials(surfAt, T.lensCount, T.halfSensor, o0, d); });
}

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
template <bool ROWS>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_differentials_kernel(
    const KolbTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out)
{
    __shared__ __align__(16) float2 lut[kLutEntries];
    stage_lut(T, lut);
    differentials_pass<ROWS, false, false>([&](float4 s, uint32_t a, uint64_t i) { return kolb_ray(T, B, lut, s, a, rngStates, rayBase, i); },
                                           samples, inputs7, nullptr, rays, n, dsx, dsy, out, nullptr);
}

template <bool ROWS>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void thin_differentials_kernel(
    const ThinTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out)
{
    differentials_pass<ROWS, false, false>([&](float4 s, uint32_t a, uint64_t i) { return thin_ray(T, B, s, a, rngStates, rayBase, i); },
                                           samples, inputs7, nullptr, rays, n, dsx, dsy, out, nullptr);
}

namespace {
template <bool ROWS>
int launch_differentials(int model, const KolbTable &kolb, const ThinTable &thin, const BokehTables &bokeh, const float *in,
                         const uint32_t *d_rng, uint64_t rayBase, uint64_t n, const RayRecord *rays, float dsx, float dsy, float *out,
                         void *stream)
{
    if (n == 0) return 0;
    const float4 *samples = ROWS ? nullptr : reinterpret_cast<const float4 *>(in);
    const float *inputs7 = ROWS ? in : nullptr;
    const uint4 *rng = reinterpret_cast<const uint4 *>(d_rng);
    if (model == 1)
        return launch_pass(kolb_differentials_kernel<ROWS>, pass_grid(n), stream, kolb, bokeh, samples, inputs7, rng, rayBase, n, rays, dsx, dsy, out);
    return launch_pass(thin_differentials_kernel<ROWS>, pass_grid(n), stream, thin, bokeh, samples, inputs7, rng, rayBase, n, rays, dsx, dsy, out);
}
}  // namespace

int launch_ray_differentials(int model, const KolbTable &kolb, const ThinTable &thin, const BokehTables &bokeh, const float *d_samples,
                             const uint32_t *d_rng, uint64_t rayBase, uint64_t n, const RayRecord *rays, float dsx, float dsy,
                             float *d_out, void *stream)
{
    return launch_differentials<false>(model, kolb, thin, bokeh, d_samples, d_rng, rayBase, n, rays, dsx, dsy, d_out, stream);
}

int launch_expand_outputs_differentials(int model, const KolbTable &kolb, const ThinTable &thin, const BokehTables &bokeh,
                                        const float *d_inputs7, uint64_t rayBase, uint64_t n, const RayRecord *rays, float *d_out21,
                                        void *stream)
{
    return launch_differentials<true>(model, kolb, thin, bokeh, d_inputs7, nullptr, rayBase, n, rays, 1.0f, 1.0f, d_out21, stream);
}

}  // namespace zoic

// differentials.hip -- the traced ray differentials (differentials.hpp): one pass over the records a ray launch wrote.
//
// Mapping: one ray per lane, wave64, 256-lane workgroups, a grid of at most 2048 workgroups striding over the batch a wave
// (64 consecutive rays) at a time.  Tables arrive as by-value kernel arguments, as in the ray kernels: the interfaces are read
// with scalar loads at a wave-uniform index.  A wave first reads the second half of its 64 records (weight, flags): if every
// weight is 0 -- 79 % of a wide-open PETZVAL frame's rays -- it writes zeros and never reads a sample; otherwise only the live
// lanes read theirs, replay their retry stream up to the accepted try (the loop runs to the wave's largest try count), rebuild
// the lens point and trace one try with two tangents.  Results leave through a per-wave LDS transpose: the 48-byte outputs of a
// wave are three fully coalesced 16-byte stores per lane (Arnold rows: 21 coalesced dword stores).
#include <hip/hip_runtime.h>

#include "differentials_device.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// RAYTRACED: the accepted try's start (differentials_device.hpp), then one traced try with tangents
__device__ __forceinline__ RayDifferential kolb_ray(const KolbTable &T, const BokehTables &B, const float2 *lut, float4 s, uint32_t a,
                                                    const uint4 *rngStates, uint64_t rayBase, uint64_t i)
{
    const auto surfAt = [&](int k) { return T.surf[__builtin_amdgcn_readfirstlane(k)]; };   // wave-uniform: scalar loads
    return kolb_replay(T, B, lut, s, a, rngStates, rayBase, i, [&](V3 o0, V3 d) { return kolb_differentials(surfAt, T.lensCount, T.halfSensor, o0, d); });
}

// The pass over a batch.  ROWS: inputs are AtCameraInput rows (each row's own dsx / dsy), outputs whole AtCameraOutput rows;
// otherwise (sx, sy, lensx, lensy) samples in, 12 floats out.  RayFn(sample, tries, i) -> RayDifferential.
template <bool ROWS, class RayFn>
__device__ __forceinline__ void differentials_pass(RayFn rayFn, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
                                                   const RayRecord *__restrict__ rays, uint64_t n, float dsx, float dsy, float *__restrict__ out)
{
    constexpr uint32_t K = ROWS ? 21u : 12u;   // floats per ray written
    __shared__ __align__(16) float stage[kDiffBlock / 64][64 * K];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *st = stage[wave];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + wave * 64u; base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        const float4 *rec = reinterpret_cast<const float4 *>(rays + (have ? i : base));
        const float4 r1 = rec[1];                                              // dy dz weight flags
        const float4 r0 = ROWS ? rec[0] : make_float4(0.f, 0.f, 0.f, 0.f);    // ox oy oz dx
        const bool live = have && r1.z != 0.0f;
        RayDifferential g{V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
        if (__ballot(live) != 0ull && live) {
            float4 s;
            float sdx = dsx, sdy = dsy;
            if constexpr (ROWS) {
                const float *p = inputs7 + i * 7u;   // sx sy dsx dsy lensx lensy relative_time
                s = make_float4(p[0], p[1], p[4], p[5]);
                sdx = p[2]; sdy = p[3];
            } else {
                s = samples[i];
            }
            g = rayFn(s, (__builtin_bit_cast(uint32_t, r1.w) >> 1) & 31u, i);
            g.dOdx = diff_scale(g.dOdx, sdx); g.dDdx = diff_scale(g.dDdx, sdx);
            g.dOdy = diff_scale(g.dOdy, sdy); g.dDdy = diff_scale(g.dDdy, sdy);
        }
        const uint64_t left = n - base;
        const uint32_t valid = left < 64u ? static_cast<uint32_t>(left) : 64u;
        if constexpr (ROWS) {
            // AtCameraOutput: origin, dir, dOdx, dOdy, dDdx, dDdy, weight[3] -- origin / dir / weight as expand_outputs_kernel copies them
            const float v[K] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, g.dOdx.x, g.dOdx.y, g.dOdx.z, g.dOdy.x, g.dOdy.y, g.dOdy.z,
                                g.dDdx.x, g.dDdx.y, g.dDdx.z, g.dDdy.x, g.dDdy.y, g.dDdy.z, r1.z, r1.z, r1.z};
#pragma unroll
            for (uint32_t f = 0; f < K; ++f) st[lane * K + f] = v[f];   // stride 21 dwords: conflict-free
        } else {
            float4 *st4 = reinterpret_cast<float4 *>(st);
            st4[lane * 3u + 0u] = make_float4(g.dOdx.x, g.dOdx.y, g.dOdx.z, g.dOdy.x);
            st4[lane * 3u + 1u] = make_float4(g.dOdy.y, g.dOdy.z, g.dDdx.x, g.dDdx.y);
            st4[lane * 3u + 2u] = make_float4(g.dDdx.z, g.dDdy.x, g.dDdy.y, g.dDdy.z);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes have landed
        if constexpr (ROWS) {
            float *dst = out + base * K;
#pragma unroll
            for (uint32_t m = 0; m < K; ++m) {
                const uint32_t j = m * 64u + lane;
                if (j < valid * K) dst[j] = st[j];
            }
        } else {
            const float4 *st4 = reinterpret_cast<const float4 *>(st);
            float4 *dst = reinterpret_cast<float4 *>(out) + base * 3u;
#pragma unroll
            for (uint32_t m = 0; m < 3u; ++m) {
                const uint32_t j = m * 64u + lane;
                if (j < valid * 3u) dst[j] = st4[j];
            }
        }
        __builtin_amdgcn_wave_barrier();   // the next wave-tile overwrites the stage
    }
}

}  // namespace

// budget: 0 scratch, 0 spills, <= 128 VGPRs (4 waves per SIMD)
template <bool ROWS>
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(4))) void kolb_differentials_kernel(
    const KolbTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out)
{
    __shared__ __align__(16) float2 lut[kLutEntries];   // (maxScale, centroid.x) pairs of the exit-pupil LUT: setup_ray's lookup
    if (threadIdx.x < kLutEntries) lut[threadIdx.x] = make_float2(T.lutMaxScale[threadIdx.x], T.lutCentroidX[threadIdx.x]);
    __syncthreads();
    differentials_pass<ROWS>([&](float4 s, uint32_t a, uint64_t i) { return kolb_ray(T, B, lut, s, a, rngStates, rayBase, i); },
                             samples, inputs7, rays, n, dsx, dsy, out);
}

template <bool ROWS>
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(4))) void thin_differentials_kernel(
    const ThinTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out)
{
    differentials_pass<ROWS>([&](float4 s, uint32_t a, uint64_t i) { return thin_ray(T, B, s, a, rngStates, rayBase, i); },
                             samples, inputs7, rays, n, dsx, dsy, out);
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
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (model == 1)
        hipLaunchKernelGGL(kolb_differentials_kernel<ROWS>, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, kolb, bokeh, samples, inputs7, rng,
                           rayBase, n, rays, dsx, dsy, out);
    else
        hipLaunchKernelGGL(thin_differentials_kernel<ROWS>, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, thin, bokeh, samples, inputs7, rng,
                           rayBase, n, rays, dsx, dsy, out);
    return static_cast<int>(hipGetLastError());
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

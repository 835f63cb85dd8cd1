// spectral_differentials.hip -- the traced ray differentials of spectral records (differentials_spectral.hpp): one pass over the
// records zoic_create_rays_spectral_device wrote.
//
// Mapping as differentials.hip: one ray per lane, wave64, 256-lane workgroups, a grid of at most 2048 workgroups striding over the
// batch a wave (64 consecutive rays) at a time; the all-dead-wave shortcut; the replay of the accepted try (differentials_device.hpp);
// results through a per-wave LDS transpose.  A lane reads one more dword, its wavelength: a lane whose wavelength is invalid is not
// live, whatever its record says.  The dispersion table arrives by value like the interfaces and is read through the kernel-argument
// segment (spectral.hpp ZOIC_SPEC_PIN) with scalar loads at the wave-uniform interface index.  CHROMATIC: the wavelength tangent is
// traced in f64 after the screen tangents (kolb_wavelength_tangent) and its six floats leave through the same transpose as three
// coalesced 8-byte stores per lane.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "differentials_device.hpp"
#include "differentials_spectral.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// The Kolb kernel's argument list as a struct (HIP lays kernel arguments out like a C struct, kolb_pool_body.hpp KolbKernelArgs)
struct SpectralDiffKernelArgs {
    KolbTable T; SpectralTable W; BokehTables B; const float4 *samples; const float *lambdas; const uint4 *rngStates; uint64_t rayBase; uint64_t n;
    const RayRecord *rays; float dsx; float dsy; float *out; float *chroma;
};
typedef const SpectralTable __attribute__((address_space(4))) *SpectralTablePtr;
__device__ __forceinline__ SpectralTablePtr kernarg_spectral()
{
    typedef const char __attribute__((address_space(4))) *KernargBytes;
    return (SpectralTablePtr)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpectralDiffKernelArgs, W));
}

// The pass over a batch: (sx, sy, lensx, lensy) samples and wavelengths in, 12 floats out, and with CHROMATIC six more to `chroma`.
// RayFn(sample, lambda, tries, i) -> SpectralDifferential.
template <bool CHROMATIC, class RayFn>
__device__ __forceinline__ void spectral_differentials_pass(RayFn rayFn, const float4 *__restrict__ samples, const float *__restrict__ lambdas,
                                                            const RayRecord *__restrict__ rays, uint64_t n, float dsx, float dsy,
                                                            float *__restrict__ out, float *__restrict__ chroma)
{
    constexpr uint32_t K = CHROMATIC ? 18u : 12u;   // floats per ray written: a wave's stage is 64 x 12, then 64 x 6
    __shared__ __align__(16) float stage[kDiffBlock / 64][64 * K];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *st = stage[wave];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDiffBlock;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kDiffBlock + wave * 64u; base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        const float4 *rec = reinterpret_cast<const float4 *>(rays + (have ? i : base));
        const float4 r1 = rec[1];                                              // dy dz weight flags
        const bool ray = have && r1.z != 0.0f;
        const float lambda = ray ? lambdas[i] : 0.0f;                          // (0: not a wavelength) a dead wave reads none
        const bool live = ray && spectral_valid(lambda);
        const V3 zero{0.f, 0.f, 0.f};
        SpectralDifferential g{RayDifferential{zero, zero, zero, zero}, zero, zero};
        if (__ballot(live) != 0ull && live) {
            g = rayFn(samples[i], lambda, (__builtin_bit_cast(uint32_t, r1.w) >> 1) & 31u, i);
            RayDifferential &r = g.screen;
            r.dOdx = diff_scale(r.dOdx, dsx); r.dDdx = diff_scale(r.dDdx, dsx);
            r.dOdy = diff_scale(r.dOdy, dsy); r.dDdy = diff_scale(r.dDdy, dsy);
        }
        const uint64_t left = n - base;
        const uint32_t valid = left < 64u ? static_cast<uint32_t>(left) : 64u;
        float4 *st4 = reinterpret_cast<float4 *>(st);
        float2 *st2 = reinterpret_cast<float2 *>(st + 64u * 12u);
        st4[lane * 3u + 0u] = make_float4(g.screen.dOdx.x, g.screen.dOdx.y, g.screen.dOdx.z, g.screen.dOdy.x);
        st4[lane * 3u + 1u] = make_float4(g.screen.dOdy.y, g.screen.dOdy.z, g.screen.dDdx.x, g.screen.dDdx.y);
        st4[lane * 3u + 2u] = make_float4(g.screen.dDdx.z, g.screen.dDdy.x, g.screen.dDdy.y, g.screen.dDdy.z);
        if constexpr (CHROMATIC) {
            st2[lane * 3u + 0u] = make_float2(g.dOdl.x, g.dOdl.y);
            st2[lane * 3u + 1u] = make_float2(g.dOdl.z, g.dDdl.x);
            st2[lane * 3u + 2u] = make_float2(g.dDdl.y, g.dDdl.z);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes have landed
        float4 *dst = reinterpret_cast<float4 *>(out) + base * 3u;
#pragma unroll
        for (uint32_t m = 0; m < 3u; ++m) {
            const uint32_t j = m * 64u + lane;
            if (j < valid * 3u) dst[j] = st4[j];
        }
        if constexpr (CHROMATIC) {
            float2 *dst2 = reinterpret_cast<float2 *>(chroma) + base * 3u;
#pragma unroll
            for (uint32_t m = 0; m < 3u; ++m) {
                const uint32_t j = m * 64u + lane;
                if (j < valid * 3u) dst2[j] = st2[j];
            }
        }
        __builtin_amdgcn_wave_barrier();   // the next wave-tile overwrites the stage
    }
}

}  // namespace

// budget: 0 scratch, 0 spills; <= 128 VGPRs (4 waves per SIMD) without the wavelength tangent, whose f64 trace may take more
template <bool CHROMATIC>
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(CHROMATIC ? 2 : 4))) void kolb_spectral_diff_kernel(
    const KolbTable T, const SpectralTable W, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ lambdas,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out, float *__restrict__ chroma)
{
    __shared__ __align__(16) float2 lut[kLutEntries];   // (maxScale, centroid.x) pairs of the exit-pupil LUT: setup_ray's lookup
    if (threadIdx.x < kLutEntries) lut[threadIdx.x] = make_float2(T.lutMaxScale[threadIdx.x], T.lutCentroidX[threadIdx.x]);
    __syncthreads();
    spectral_differentials_pass<CHROMATIC>(
        [&](float4 s, float lambda, uint32_t a, uint64_t i) {
            const auto surfAt = [&](int k) { return T.surf[__builtin_amdgcn_readfirstlane(k)]; };   // wave-uniform: scalar loads
            return kolb_replay(T, B, lut, s, a, rngStates, rayBase, i, [&](V3 o0, V3 d) {
                return kolb_differentials_spectral<CHROMATIC>(surfAt, kernarg_spectral(), T.lensCount, lambda, T.halfSensor, o0, d);
            });
        },
        samples, lambdas, rays, n, dsx, dsy, out, chroma);
}

// THINLENS: the wavelength only rejects
template <bool CHROMATIC>
__global__ __launch_bounds__(kDiffBlock) __attribute__((amdgpu_waves_per_eu(4))) void thin_spectral_diff_kernel(
    const ThinTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ lambdas,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out, float *__restrict__ chroma)
{
    spectral_differentials_pass<CHROMATIC>(
        [&](float4 s, float, uint32_t a, uint64_t i) {
            return SpectralDifferential{thin_ray(T, B, s, a, rngStates, rayBase, i), V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
        },
        samples, lambdas, rays, n, dsx, dsy, out, chroma);
}

namespace {
template <bool CHROMATIC>
int launch_spectral_diff(int model, const KolbTable &kolb, const SpectralTable &spec, const ThinTable &thin, const BokehTables &bokeh,
                         const float4 *samples, const float *d_lambda, const uint4 *rng, uint64_t rayBase, uint64_t n, const RayRecord *rays,
                         float dsx, float dsy, float *out, float *chroma, hipStream_t s)
{
    if (model == 1)
        hipLaunchKernelGGL(kolb_spectral_diff_kernel<CHROMATIC>, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, kolb, spec, bokeh, samples, d_lambda,
                           rng, rayBase, n, rays, dsx, dsy, out, chroma);
    else
        hipLaunchKernelGGL(thin_spectral_diff_kernel<CHROMATIC>, dim3(diff_grid(n)), dim3(kDiffBlock), 0, s, thin, bokeh, samples, d_lambda, rng,
                           rayBase, n, rays, dsx, dsy, out, chroma);
    return static_cast<int>(hipGetLastError());
}
}  // namespace

int launch_ray_differentials_spectral(int model, const KolbTable &kolb, const SpectralTable &spec, const ThinTable &thin,
                                      const BokehTables &bokeh, const float *d_samples, const float *d_lambda, const uint32_t *d_rng,
                                      uint64_t rayBase, uint64_t n, const RayRecord *rays, float dsx, float dsy, float *d_out,
                                      float *d_chromatic, void *stream)
{
    if (n == 0) return 0;
    const float4 *samples = reinterpret_cast<const float4 *>(d_samples);
    const uint4 *rng = reinterpret_cast<const uint4 *>(d_rng);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    return d_chromatic ? launch_spectral_diff<true>(model, kolb, spec, thin, bokeh, samples, d_lambda, rng, rayBase, n, rays, dsx, dsy, d_out, d_chromatic, s)
                       : launch_spectral_diff<false>(model, kolb, spec, thin, bokeh, samples, d_lambda, rng, rayBase, n, rays, dsx, dsy, d_out, nullptr, s);
}

}  // namespace zoic

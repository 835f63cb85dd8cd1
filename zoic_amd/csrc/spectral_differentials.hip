// spectral_differentials.hip -- the traced ray differentials of spectral records (differentials_spectral.hpp): one pass over the
// records zoic_create_rays_spectral_device wrote.
//
// Mapping as differentials.hip, through the same pass (record_pass.hpp differentials_pass with SPECTRAL).  A lane reads one more dword,
// its wavelength: a lane whose wavelength is invalid is not live, whatever its record says.  The dispersion table arrives by value like
// the interfaces and is read through the kernel-argument segment (device_pass.hpp kernarg_view, spectral.hpp ZOIC_SPEC_PIN) with scalar
// loads at the wave-uniform interface index.  CHROMATIC: the wavelength tangent is traced in f64 after the screen tangents
// (kolb_wavelength_tangent) and its six floats leave through the same stage as three coalesced 8-byte stores per lane.
#include <hip/hip_runtime.h>

#include "record_pass.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

// the Kolb kernel's argument list (device_pass.hpp kernarg_view)
struct SpectralDiffKernelArgs {
    KolbTable T; SpectralTable W; BokehTables B; const float4 *samples; const float *lambdas; const uint4 *rngStates; uint64_t rayBase; uint64_t n;
    const RayRecord *rays; float dsx; float dsy; float *out; float *chroma;
};
__device__ __forceinline__ auto kernarg_spectral() { return kernarg_view<SpectralDiffKernelArgs, SpectralTable>(offsetof(SpectralDiffKernelArgs, W)); }

}  // namespace

// budget: 0 scratch, 0 spills; <= 128 VGPRs (4 waves per SIMD) without the wavelength tangent, whose f64 trace may take more
template <bool CHROMATIC>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(CHROMATIC ? 2 : 4))) void kolb_spectral_diff_kernel(
    const KolbTable T, const SpectralTable W, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ lambdas,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out, float *__restrict__ chroma)
{
    __shared__ __align__(16) float2 lut[kLutEntries];
    stage_lut(T, lut);
    differentials_pass<false, true, CHROMATIC>(
        [&](float4 s, float lambda, uint32_t a, uint64_t i) {
            const auto surfAt = [&](int k) { return T.surf[__builtin_amdgcn_readfirstlane(k)]; };   // wave-uniform: scalar loads
            return kolb_replay(T, B, lut, s, a, rngStates, rayBase, i, [&](V3 o0, V3 d) {
                return kolb_differentials_spectral<CHROMATIC>(surfAt, kernarg_spectral(), T.lensCount, lambda, T.halfSensor, o0, d);
            });
        },
        samples, nullptr, lambdas, rays, n, dsx, dsy, out, chroma);
}

// THINLENS: the wavelength only rejects
template <bool CHROMATIC>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void thin_spectral_diff_kernel(
    const ThinTable T, const BokehTables B, const float4 *__restrict__ samples, const float *__restrict__ lambdas,
    const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n, const RayRecord *__restrict__ rays, float dsx, float dsy,
    float *__restrict__ out, float *__restrict__ chroma)
{
    differentials_pass<false, true, CHROMATIC>(
        [&](float4 s, float, uint32_t a, uint64_t i) {
            return SpectralDifferential{thin_ray(T, B, s, a, rngStates, rayBase, i), V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}};
        },
        samples, nullptr, lambdas, rays, n, dsx, dsy, out, chroma);
}

namespace {
template <bool CHROMATIC>
int launch_spectral_diff(int model, const KolbTable &kolb, const SpectralTable &spec, const ThinTable &thin, const BokehTables &bokeh,
                         const float4 *samples, const float *d_lambda, const uint4 *rng, uint64_t rayBase, uint64_t n, const RayRecord *rays,
                         float dsx, float dsy, float *out, float *chroma, void *stream)
{
    if (model == 1)
        return launch_pass(kolb_spectral_diff_kernel<CHROMATIC>, pass_grid(n), stream, kolb, spec, bokeh, samples, d_lambda, rng, rayBase, n, rays,
                           dsx, dsy, out, chroma);
    return launch_pass(thin_spectral_diff_kernel<CHROMATIC>, pass_grid(n), stream, thin, bokeh, samples, d_lambda, rng, rayBase, n, rays, dsx, dsy,
                       out, chroma);
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
    return d_chromatic ? launch_spectral_diff<true>(model, kolb, spec, thin, bokeh, samples, d_lambda, rng, rayBase, n, rays, dsx, dsy, d_out, d_chromatic, stream)
                       : launch_spectral_diff<false>(model, kolb, spec, thin, bokeh, samples, d_lambda, rng, rayBase, n, rays, dsx, dsy, d_out, nullptr, stream);
}

}  // namespace zoic

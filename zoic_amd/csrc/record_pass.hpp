// record_pass.hpp -- what the passes over records that already exist share on the device (differentials.hip,
// spectral_differentials.hip, transmittance.hip, ghost.hip; spectral.hip takes the LUT staging and the try count): the skeleton of such a
// pass, the replay of a record's accepted try with the ray kernels' own STRICT helpers, and the differentials' pass over a batch.
//
// Mapping (launch shape: device_pass.hpp): one sample per lane, a wave taking 64 consecutive samples -- a wave-tile -- at a time and the
// grid striding over the batch.  A pass reads weight and flags of its records, finds the live lanes (a wave without one never reads a
// sample), replays the accepted try once per live sample and writes through a per-wave LDS stage as fully coalesced stores.
#pragma once
#include <hip/hip_runtime.h>

#include "device_pass.hpp"
#include "differentials_spectral.hpp"
#include "kolb_pool_body.hpp"
#include "thin_device.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// (maxScale, centroid.x) pairs of the exit-pupil LUT into the workgroup's LDS: setup_ray's lookup
static __device__ __forceinline__ void stage_lut(const KolbTable &T, float2 (&lut)[kLutEntries])
{
    if (threadIdx.x < kLutEntries) lut[threadIdx.x] = make_float2(T.lutMaxScale[threadIdx.x], T.lutCentroidX[threadIdx.x]);
    __syncthreads();
}

// The wave-tile walk of a pass:
//     for (uint64_t base = first_wave_tile(); base < n; base += stride)      with stride = pass_stride()
// and in it i = base + lane, have = i < n (a lane past the end stays with its wave).  The loop is written out in each pass: handed to
// a helper as a lambda body it compiled to other code in all three passes and measured slower in the transmittance and ghost kernels.
static __device__ __forceinline__ uint64_t first_wave_tile()
{
    return static_cast<uint64_t>(blockIdx.x) * kPassBlock + (threadIdx.x >> 6) * 64u;
}

// the accepted try of a record, from its flag word
ZOIC_HD uint32_t record_tries(uint32_t flags) { return (flags >> 1) & 31u; }

// The lanes of a wave have written the tile's values into the wave's stage: the first valid x perLane elements (float, float2 or
// float4) leave for dst as coalesced stores.  The closing barrier: the next wave-tile overwrites the stage.
template <class E>
static __device__ __forceinline__ void staged_store(const E *stage, E *__restrict__ dst, uint32_t valid, uint32_t perLane)
{
    const uint32_t lane = threadIdx.x & 63u;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS writes have landed
    for (uint32_t m = 0; m < perLane; ++m) {
        const uint32_t j = m * 64u + lane;
        if (j < valid * perLane) dst[j] = stage[j];
    }
    __builtin_amdgcn_wave_barrier();
}

// samples of the wave-tile at `base` that exist
static __device__ __forceinline__ uint32_t tile_valid(uint64_t n, uint64_t base)
{
    const uint64_t left = n - base;
    return left < 64u ? static_cast<uint32_t>(left) : 64u;
}

// The lens-sample draw of the accepted try a: (lensx, lensy) for a == 0, else draws 2a-1 and 2a of the ray's retry stream
// (zoic.cpp:1930 / 1806: the order every ray kernel draws them in).  The stream is the caller's state or rng_for_ray(seed, index).
static __device__ __forceinline__ V2 accepted_draw(float4 s, uint32_t a, const uint4 *rngStates, uint32_t seed, uint64_t rayIndex, uint64_t i)
{
    Rng rng{1u, 2u, 3u, 4u};
    if (a > 0u) {
        if (rngStates) { const uint4 r = rngStates[i]; rng = Rng{r.x, r.y, r.z, r.w}; }
        else rng = rng_for_ray(seed, rayIndex);
    }
    for (uint32_t k = 1; __ballot(k < a) != 0ull; ++k) {   // tries 1 .. a-1 were rejected: step over their draws
        if (k < a) { (void)xor128(rng); (void)xor128(rng); }
    }
    if (a == 0u) return V2{s.z, s.w};
    const float u = rng_unit(xor128(rng));
    const float v = rng_unit(xor128(rng));
    return V2{u, v};
}

// RAYTRACED: the accepted try's start (zoic.cpp:1853-1943, the ray kernels' STRICT set-up), then trace(o0, d): the sensor point and
// the direction to the lens point -> what the pass returns for the ray
template <class Trace>
static __device__ __forceinline__ auto kolb_replay(const KolbTable &T, const BokehTables &B, const float2 *lut, float4 s, uint32_t a,
                                                   const uint4 *rngStates, uint64_t rayBase, uint64_t i, Trace trace)
{
    const RaySetup rs = setup_ray<true>(T, lut, s.x, s.y);
    const V2 draw = accepted_draw(s, a, rngStates, T.seed, rayBase + i, i);
    V2 lens = lens_sample<true>(T, B, nullptr, draw.x, draw.y);
    V3 d;
    if (a > 0u) {
        d = retry_direction(T, lens, rs.o0x, rs.o0y, rs.maxScale, rs.translation, rs.sn, rs.cs);   // zoic.cpp:1932-1943
    } else if (!T.useLUT) {
        d = V3{(lens.x * T.rearAperture) - rs.o0x, (lens.y * T.rearAperture) - rs.o0y, T.dirZ};   // zoic.cpp:1873-1877
    } else {                                                                                    // zoic.cpp:1913-1924
        lens.x *= rs.maxScale; lens.y *= rs.maxScale;
        lens.x += rs.translation;
        const float rx = lens.x * rs.cs - lens.y * rs.sn, ry = lens.x * rs.sn + lens.y * rs.cs;
        d = V3{rx - rs.o0x, ry - rs.o0y, T.dirZ};
    }
    return trace(V3{rs.o0x, rs.o0y, T.originShift}, d);
}

// the start (o0, d0) of the accepted try, for the passes that trace from it themselves
static __device__ __forceinline__ void accepted_start(const KolbTable &T, const BokehTables &B, const float2 *lut, float4 s, uint32_t a,
                                                      const uint4 *rngStates, uint64_t rayBase, uint64_t i, V3 &o0, V3 &d0)
{
    kolb_replay(T, B, lut, s, a, rngStates, rayBase, i, [&](V3 o, V3 d) { o0 = o; d0 = d; return 0; });
}

// THINLENS (zoic.cpp:1771-1846): the accepted try's lens point is the origin; p |focalDistance| is restated as the reference
// computes it (dir0 * |focalDistance / dir0.z|)
static __device__ __forceinline__ RayDifferential thin_ray(const ThinTable &T, const BokehTables &B, float4 s, uint32_t a, const uint4 *rngStates,
                                                    uint64_t rayBase, uint64_t i)
{
    const V3 p{s.x * T.tanFov, s.y * T.tanFov, 1.0f};
    if (!T.useDof) return thin_differentials(p, T.tanFov);
    const V2 draw = accepted_draw(s, a, rngStates, T.seed, rayBase + i, i);
    const V2 lens = sample_lens(T.useImage != 0, B, nullptr, T.bokehW, T.bokehH, draw.x, draw.y);
    const V3 dir0 = normalize3(p);
    const float inter = fabsf(T.focalDistance / dir0.z);
    const V3 q{dir0.x * inter - lens.x * T.apertureRadius, dir0.y * inter - lens.y * T.apertureRadius, dir0.z * inter};
    return thin_differentials(q, T.tanFov * fabsf(T.focalDistance));
}

// The differentials' pass over a batch.  A wave first reads the second half of its records (weight, flags) and, with SPECTRAL, the
// wavelengths of the rays that have weight -- a lane whose wavelength is invalid is not live, whatever its record says.  A wave without
// a live lane writes zeros and never reads a sample; otherwise the live lanes call rayFn and scale its tangents by dsx / dsy.
//   ROWS: inputs are AtCameraInput rows (each row's own dsx / dsy), outputs whole AtCameraOutput rows (21 dword stores per lane);
//   otherwise (sx, sy, lensx, lensy) samples in, 12 floats out (three 16-byte stores per lane), and with CHROMATIC six more to
//   `chroma` (three 8-byte stores per lane).
// RayFn(sample, tries, i) -> RayDifferential, with SPECTRAL RayFn(sample, lambda, tries, i) -> SpectralDifferential.
template <bool ROWS, bool SPECTRAL, bool CHROMATIC, class RayFn>
static __device__ __forceinline__ void differentials_pass(RayFn rayFn, const float4 *__restrict__ samples, const float *__restrict__ inputs7,
                                                          const float *__restrict__ lambdas, const RayRecord *__restrict__ rays, uint64_t n,
                                                          float dsx, float dsy, float *__restrict__ out, float *__restrict__ chroma)
{
    static_assert(!(ROWS && SPECTRAL) && (SPECTRAL || !CHROMATIC), "Arnold rows carry no wavelength; the wavelength tangent needs one");
    constexpr uint32_t K = ROWS ? 21u : CHROMATIC ? 18u : 12u;   // floats per ray written (CHROMATIC: a wave's stage is 64 x 12, then 64 x 6)
    __shared__ __align__(16) float stage[kPassBlock / 64][64 * K];
    float *st = stage[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = pass_stride();
    for (uint64_t base = first_wave_tile(); base < n; base += stride) {
        const uint64_t i = base + lane;
        const bool have = i < n;
        const float4 *rec = reinterpret_cast<const float4 *>(rays + (have ? i : base));
        const float4 r1 = rec[1];                                              // dy dz weight flags
        const float4 r0 = ROWS ? rec[0] : make_float4(0.f, 0.f, 0.f, 0.f);    // ox oy oz dx
        bool live = have && r1.z != 0.0f;
        float lambda = 0.0f;
        if constexpr (SPECTRAL) {
            if (live) lambda = lambdas[i];                                     // (0: not a wavelength) a dead wave reads none
            live = live && spectral_valid(lambda);
        }
        const V3 zero{0.f, 0.f, 0.f};
        SpectralDifferential g{RayDifferential{zero, zero, zero, zero}, zero, zero};
        RayDifferential &r = g.screen;
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
            const uint32_t tries = record_tries(__builtin_bit_cast(uint32_t, r1.w));
            if constexpr (SPECTRAL) g = rayFn(s, lambda, tries, i);
            else r = rayFn(s, tries, i);
            r.dOdx = diff_scale(r.dOdx, sdx); r.dDdx = diff_scale(r.dDdx, sdx);
            r.dOdy = diff_scale(r.dOdy, sdy); r.dDdy = diff_scale(r.dDdy, sdy);
        }
        const uint32_t valid = tile_valid(n, base);
        if constexpr (ROWS) {
            // AtCameraOutput: origin, dir, dOdx, dOdy, dDdx, dDdy, weight[3] -- origin / dir / weight as expand_outputs_kernel copies them
            const float v[K] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r.dOdx.x, r.dOdx.y, r.dOdx.z, r.dOdy.x, r.dOdy.y, r.dOdy.z,
                                r.dDdx.x, r.dDdx.y, r.dDdx.z, r.dDdy.x, r.dDdy.y, r.dDdy.z, r1.z, r1.z, r1.z};
#pragma unroll
            for (uint32_t f = 0; f < K; ++f) st[lane * K + f] = v[f];   // stride 21 dwords: conflict-free
            staged_store(st, out + base * K, valid, K);
        } else {
            float4 *st4 = reinterpret_cast<float4 *>(st);
            st4[lane * 3u + 0u] = make_float4(r.dOdx.x, r.dOdx.y, r.dOdx.z, r.dOdy.x);
            st4[lane * 3u + 1u] = make_float4(r.dOdy.y, r.dOdy.z, r.dDdx.x, r.dDdx.y);
            st4[lane * 3u + 2u] = make_float4(r.dDdx.z, r.dDdy.x, r.dDdy.y, r.dDdy.z);
            float2 *st2 = reinterpret_cast<float2 *>(st + 64u * 12u);
            if constexpr (CHROMATIC) {
                st2[lane * 3u + 0u] = make_float2(g.dOdl.x, g.dOdl.y);
                st2[lane * 3u + 1u] = make_float2(g.dOdl.z, g.dDdl.x);
                st2[lane * 3u + 2u] = make_float2(g.dDdl.y, g.dDdl.z);
            }
            staged_store(st4, reinterpret_cast<float4 *>(out) + base * 3u, valid, 3u);
            if constexpr (CHROMATIC) staged_store(st2, reinterpret_cast<float2 *>(chroma) + base * 3u, valid, 3u);
        }
    }
}

}  // namespace zoic

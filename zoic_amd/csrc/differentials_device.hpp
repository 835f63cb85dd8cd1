// differentials_device.hpp -- what the differential passes (differentials.hip, spectral_differentials.hip) share on the device:
// the launch shape and the replay of a record's accepted try with the ray kernels' own STRICT helpers.
#pragma once
#include <hip/hip_runtime.h>

#include "differentials.hpp"
#include "kolb_pool_body.hpp"
#include "thin_device.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr int kDiffBlock = 256;
constexpr uint64_t kDiffGridCap = 2048;

inline uint32_t diff_grid(uint64_t n)
{
    const uint64_t blocks = (n + kDiffBlock - 1) / kDiffBlock;
    return static_cast<uint32_t>(blocks < kDiffGridCap ? blocks : kDiffGridCap);
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

}  // namespace zoic

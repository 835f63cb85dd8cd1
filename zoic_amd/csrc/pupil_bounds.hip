// pupil_bounds.hip -- the batch pupil bounds (pupil_bounds.hpp), d-line and at a wavelength per point: two kernels (an instance per lens
// model), one scene point per wave.
//
// Mapping: the launch shape of device_pass.hpp with a wave's point as the item, so four points per workgroup per step; the waves walk
// a larger batch with a grid stride.  The TraceBackTable (and, spectral, the BackwardDispersion) arrives by value as a kernel
// argument, and so do the lattice and the window: everything but the aim is wave-uniform, the interface loop's index included, so
// every table entry stays one scalar load.  The point (12 bytes) and, spectral, its wavelength are loaded once per wave at a
// wave-uniform address.  Lane l traces the aims l, l + 64, ...: G^2 / 64 of them, the same trip count in every lane, and keeps ten
// running values (four aim minima / maxima, four screen minima / maxima, a count, a reason mask).  A lane whose ray has ended waits
// for the wave's interface loop, as in traceback.hip.  Then the 64 partial results are merged by a butterfly of __shfl_xor (ds_bpermute:
// no LDS allocation), six rounds of ten values, after which every lane holds the wave's result and lane 0 writes the 48-byte record as
// three 16-byte stores.  No atomics, no scratch, no early return before the reduction; a wave whose point index is >= n skips the
// whole body by a wave-uniform branch, and nothing is read or written past n.
#include <hip/hip_runtime.h>

#include "device_pass.hpp"
#include "pupil_bounds.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr int kPbWaves = kPassBlock / 64;   // points per workgroup per step

__device__ __forceinline__ float pb_xor(float v, int off) { return __shfl_xor(v, off, 64); }
__device__ __forceinline__ uint32_t pb_xor(uint32_t v, int off) { return static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off, 64)); }

// the wave's result in every lane
__device__ __forceinline__ void pb_reduce(PupilAcc &A)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        PupilAcc B;
        B.axMin = pb_xor(A.axMin, off); B.ayMin = pb_xor(A.ayMin, off); B.axMax = pb_xor(A.axMax, off); B.ayMax = pb_xor(A.ayMax, off);
        B.sxMin = pb_xor(A.sxMin, off); B.syMin = pb_xor(A.syMin, off); B.sxMax = pb_xor(A.sxMax, off); B.syMax = pb_xor(A.syMax, off);
        B.count = pb_xor(A.count, off); B.reasons = pb_xor(A.reasons, off);
        pupil_merge(A, B);
    }
}

// the grid-stride walk of both kernels: trace(p, ox, oy, oz, dx, dy, dz, sx, sy) returns the flag word of one ray from point p
template <class Trace>
__device__ __forceinline__ void pb_walk(const TraceBackTable &T, const float *__restrict__ points, uint64_t n, int shift, const PupilWindow &W,
                                        float4 *__restrict__ bounds, Trace trace)
{
    const int lane = static_cast<int>(threadIdx.x & 63u);
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));   // wave-uniform, provably
    const PupilFrame F = pupil_frame(T, 1 << shift);
    const int trips = 1 << (2 * shift - 6);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kPbWaves;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * kPbWaves + wave; p < n; p += stride) {
        const float px = points[3u * p], py = points[3u * p + 1u], pz = points[3u * p + 2u];
        PupilAcc A;
        for (int k = 0; k < trips; ++k)
            pupil_aim(A, F, shift, lane + 64 * k, px, py, pz, W, [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
                return trace(p, ox, oy, oz, dx, dy, dz, sx, sy);
            });
        pb_reduce(A);
        const PupilBounds B = pupil_record(A, F, shift);
        if (lane == 0) {
            bounds[3u * p] = make_float4(B.aim[0], B.aim[1], B.aim[2], B.aim[3]);
            bounds[3u * p + 1u] = make_float4(B.screen[0], B.screen[1], B.screen[2], B.screen[3]);
            bounds[3u * p + 2u] = make_float4(__uint_as_float(B.count), __uint_as_float(B.lattice), __uint_as_float(B.flags), __uint_as_float(B.reserved));
        }
    }
}

}  // namespace

// The lens model is a template parameter (traceback.hpp assume_model / model_instance).
// budget (all six): 0 scratch, 0 spills, 0 LDS
template <int kModel>
__global__ __launch_bounds__(kPassBlock) void pupil_bounds_kernel(const TraceBackTable T, const float *__restrict__ points, uint64_t n, int shift,
                                                                const PupilWindow W, float4 *__restrict__ bounds)
{
    assume_model<kModel>(T);
    pb_walk(T, points, n, shift, W, bounds, [&](uint64_t, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray(T, ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

template <int kModel>
__global__ __launch_bounds__(kPassBlock) void pupil_bounds_spectral_kernel(const TraceBackTable T, const BackwardDispersion D,
                                                                         const float *__restrict__ points, const float *__restrict__ lambda,
                                                                         uint64_t n, int shift, const PupilWindow W, float4 *__restrict__ bounds)
{
    assume_model<kModel>(T);
    pb_walk(T, points, n, shift, W, bounds, [&](uint64_t p, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray_spectral(T, D, lambda[p], ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

int launch_pupil_bounds(const TraceBackTable &T, const float *d_points, uint64_t n, int G, const PupilWindow &W, void *d_bounds, void *stream)
{
    if (n == 0) return 0;
    if (!pupil_lattice_valid(G)) return static_cast<int>(hipErrorInvalidValue);
    const auto kernel = model_instance(T, pupil_bounds_kernel<kModelThin>, pupil_bounds_kernel<kModelKolb>, pupil_bounds_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(n, kPbWaves), stream, T, d_points, n, pupil_shift(G), W, static_cast<float4 *>(d_bounds));
}

int launch_pupil_bounds_spectral(const TraceBackTable &T, const BackwardDispersion &D, const float *d_points, const float *d_lambda, uint64_t n,
                                 int G, const PupilWindow &W, void *d_bounds, void *stream)
{
    if (n == 0) return 0;
    if (!pupil_lattice_valid(G)) return static_cast<int>(hipErrorInvalidValue);
    const auto kernel = model_instance(T, pupil_bounds_spectral_kernel<kModelThin>, pupil_bounds_spectral_kernel<kModelKolb>,
                                       pupil_bounds_spectral_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(n, kPbWaves), stream, T, D, d_points, d_lambda, n, pupil_shift(G), W, static_cast<float4 *>(d_bounds));
}

}  // namespace zoic

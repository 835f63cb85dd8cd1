// traceback_throughput.hip -- the batch trace-back transmittance (traceback_throughput.hpp), ray side and splat side: two kernels (an instance
// per lens model each), one ray per lane.
//
// Mapping: the launch shape and the one-item-per-lane walk of device_pass.hpp.  The TraceBackTable, the BackwardDispersion and the
// FilmTable arrive by value as kernel arguments (about 1.1 KB): the interface index is wave-uniform, so the surface entry, the medium
// entry and the two film entries of an interface are scalar loads.  The wavelength pointer is a wave-uniform null test: a d-line call
// passes nullptr and every lane takes kLambdaD32, so one kernel serves both forms (a d-line kernel of its own saves two VGPRs and one
// SGPR).  The model instances (traceback.hpp assume_model) keep the other model's table fields out of the scalar registers: the one
// generic ray-side kernel spilled six of them.
//   Ray side   A lane reads its 32-byte record as traceback.hip's tb_walk does (two 16-byte loads) and, spectral, its wavelength; runs
//              the one trace with the rider; writes one float and, where the caller gave pointers, the float2 screen sample and the
//              flag word.
//   Splat side splat.hip's index walk (point p = i / m without a 64-bit division) and loads: the point, the box row and the
//              count / flags row of its pupil-bounds record, u; the trace without the Jacobian's tangents; one coalesced float per
//              lane.  A lane whose box is empty skips the trace under the exec mask and stores +0.0f.
// Multilayer coatings (coating_stack.hpp): a camera with a stack on any interface runs tb_stack_throughput_kernel /
// aim_stack_throughput_kernel under the coating policy `const StackTable *` (the camera's table in device memory, scalar loads at the
// wave-uniform interface index); RAYTRACED only -- no other model has an interface.  The ray side shares the plain kernels' body; the
// splat side takes one slab per launch without the walk (see the kernel).
// No atomics, no LDS, no scratch; nothing is read or written past n (n m).
#include <hip/hip_runtime.h>

#include "device_pass.hpp"
#include "traceback_throughput.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// The lens model is a template parameter of both kernels (traceback.hpp assume_model / model_instance); the coating policy KP
// (coating_stack.hpp) of the ray side's body is NoStacks in them and `const StackTable *` in the stack-aware kernel.
template <class KP>
__device__ __forceinline__ void tb_throughput_pass(const TraceBackTable &T, const BackwardDispersion &D, const FilmTable &F,
                                                   const float4 *__restrict__ rays, const float *__restrict__ lambda, uint64_t n,
                                                   float *__restrict__ out, float2 *__restrict__ screen, uint32_t *__restrict__ flags, KP K)
{
    for_each_item(n, [&](uint64_t i) {
        const float4 a = rays[2u * i], b = rays[2u * i + 1u];   // ox oy oz dx | dy dz weight flags
        const float l = lambda ? lambda[i] : kLambdaD32;
        float sx, sy, t;
        const uint32_t f = trace_back_ray_throughput(T, D, &F, l, a.x, a.y, a.z, a.w, b.x, b.y, sx, sy, t, K);
        out[i] = t;
        if (screen) screen[i] = make_float2(sx, sy);
        if (flags) flags[i] = f;
    });
}

// budget (all three): 0 scratch, 0 spills, 0 LDS; at most 96 VGPRs
template <int kModel>
__global__ __launch_bounds__(kPassBlock) void tb_throughput_kernel(const TraceBackTable T, const BackwardDispersion D, const FilmTable F,
                                                                 const float4 *__restrict__ rays, const float *__restrict__ lambda, uint64_t n,
                                                                 float *__restrict__ out, float2 *__restrict__ screen,
                                                                 uint32_t *__restrict__ flags)
{
    assume_model<kModel>(T);
    tb_throughput_pass(T, D, F, rays, lambda, n, out, screen, flags, NoStacks{});
}

// RAYTRACED with multilayer coatings (no other model has an interface); budget: the same
__global__ __launch_bounds__(kPassBlock) void tb_stack_throughput_kernel(const TraceBackTable T, const BackwardDispersion D, const FilmTable F,
                                                                       const float4 *__restrict__ rays, const float *__restrict__ lambda,
                                                                       uint64_t n, float *__restrict__ out, float2 *__restrict__ screen,
                                                                       uint32_t *__restrict__ flags, const StackTable *__restrict__ stacks)
{
    assume_model<kModelKolb>(T);
    tb_throughput_pass(T, D, F, rays, lambda, n, out, screen, flags, stacks);
}

// budget (all three): 0 scratch, 0 spills, 0 LDS; the RAYTRACED instance no more VGPRs than the RAYTRACED splat kernel
template <int kModel>
__global__ __launch_bounds__(kPassBlock) void aim_throughput_kernel(const TraceBackTable T, const BackwardDispersion D, const FilmTable F,
                                                                  const float *__restrict__ points, const float4 *__restrict__ bounds,
                                                                  const float *__restrict__ lambda, uint64_t total, uint32_t m,
                                                                  const float2 *__restrict__ u, float *__restrict__ out)
{
    assume_model<kModel>(T);
    const float z = splat_plane(T);
    const uint32_t stride = gridDim.x * static_cast<uint32_t>(kPassBlock);   // <= 2^19
    const uint32_t first = blockIdx.x * static_cast<uint32_t>(kPassBlock) + threadIdx.x;
    const uint32_t stepP = stride / m, stepJ = stride % m;                  // wave-uniform
    uint64_t p = first / m;
    uint32_t j = first % m;
    for (uint64_t i = first; i < total; i += stride) {
        const float px = points[3u * p], py = points[3u * p + 1u], pz = points[3u * p + 2u];
        const float4 box = bounds[3u * p], tail = bounds[3u * p + 2u];     // aim[4] | count lattice flags reserved
        const float2 uu = u[i];
        const uint32_t count = __float_as_uint(tail.x), boxFlags = __float_as_uint(tail.z);
        const float l = lambda ? lambda[p] : kLambdaD32;
        out[i] = splat_throughput(T, D, &F, l, z, px, py, pz, box.x, box.y, box.z, box.w, count, boxFlags, uu.x, uu.y);
        // i + stride = (p + stepP) m + (j + stepJ), and j + stepJ < 2 m
        p += stepP;
        if (j >= m - stepJ) { j -= m - stepJ; ++p; }
        else j += stepJ;
    }
}

// RAYTRACED with multilayer coatings; budget: the same.  ONE SLAB PER LAUNCH, no walk: under the plain kernel's grid-stride walk the
// layer loop's scalar state did not fit beside the walk's (stride, steps, total, the loop's exec mask) and the table fields the compiler
// keeps across it -- 106 SGPRs and two spilled; without the walk the kernel takes 74.  The launcher sends a batch of more than one grid's
// worth (kPassGridCap x kPassBlock items) slab by slab on the same stream.  base: the slab's first item, = pBase m + jBase with
// jBase < m; items: the slab's, at most 2^19.  The arithmetic per item is aim_throughput_kernel's.
__global__ __launch_bounds__(kPassBlock) void aim_stack_throughput_kernel(const TraceBackTable T, const BackwardDispersion D, const FilmTable F,
                                                                        const float *__restrict__ points, const float4 *__restrict__ bounds,
                                                                        const float *__restrict__ lambda, uint64_t base, uint64_t pBase,
                                                                        uint32_t jBase, uint32_t items, uint32_t m,
                                                                        const float2 *__restrict__ u, float *__restrict__ out,
                                                                        const StackTable *__restrict__ stacks)
{
    assume_model<kModelKolb>(T);
    const uint32_t first = blockIdx.x * static_cast<uint32_t>(kPassBlock) + threadIdx.x;   // < 2^19
    if (first >= items) return;
    // the point of item base + first: pBase + (jBase + first) / m.  jBase + first < m + 2^19: with m >= 2^19 the quotient is 0 or 1 (and
    // the sum may pass 2^32, hence 64 bits); otherwise the sum is below 2^20 and a 32-bit division serves.  m is wave-uniform.
    const uint64_t q = static_cast<uint64_t>(jBase) + first;
    const uint32_t step = m >= (1u << 19) ? (q >= m ? 1u : 0u) : static_cast<uint32_t>(q) / m;
    const uint64_t p = pBase + step, i = base + first;
    const float z = splat_plane(T);
    const float px = points[3u * p], py = points[3u * p + 1u], pz = points[3u * p + 2u];
    const float4 box = bounds[3u * p], tail = bounds[3u * p + 2u];     // aim[4] | count lattice flags reserved
    const float2 uu = u[i];
    const uint32_t count = __float_as_uint(tail.x), boxFlags = __float_as_uint(tail.z);
    const float l = lambda ? lambda[p] : kLambdaD32;
    out[i] = splat_throughput(T, D, &F, l, z, px, py, pz, box.x, box.y, box.z, box.w, count, boxFlags, uu.x, uu.y, stacks);
}

int launch_trace_back_throughput(const TraceBackTable &T, const BackwardDispersion &D, const FilmTable &F, const void *d_rays,
                                 const float *d_lambda, uint64_t n, float *d_out, float *d_screen, uint32_t *d_flags, void *stream,
                                 const StackTable *d_stacks)
{
    if (n == 0) return 0;
    if (d_stacks && T.model == kModelKolb)
        return launch_pass(tb_stack_throughput_kernel, pass_grid(n), stream, T, D, F, static_cast<const float4 *>(d_rays), d_lambda, n, d_out,
                           reinterpret_cast<float2 *>(d_screen), d_flags, d_stacks);
    const auto kernel = model_instance(T, tb_throughput_kernel<kModelThin>, tb_throughput_kernel<kModelKolb>, tb_throughput_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(n), stream, T, D, F, static_cast<const float4 *>(d_rays), d_lambda, n, d_out,
                       reinterpret_cast<float2 *>(d_screen), d_flags);
}

int launch_splat_throughput(const TraceBackTable &T, const BackwardDispersion &D, const FilmTable &F, const float *d_points,
                            const void *d_bounds, const float *d_lambda, uint64_t n, uint32_t m, const float *d_u, float *d_out, void *stream,
                            const StackTable *d_stacks)
{
    if (n == 0) return 0;
    if (m == 0) return static_cast<int>(hipErrorInvalidValue);
    const uint64_t total = n * m;
    if (d_stacks && T.model == kModelKolb) {
        constexpr uint64_t slab = kPassGridCap * kPassBlock;   // one grid's worth of items per launch
        for (uint64_t base = 0; base < total; base += slab) {
            const uint32_t items = static_cast<uint32_t>(total - base < slab ? total - base : slab);
            const int e = launch_pass(aim_stack_throughput_kernel, pass_grid(items), stream, T, D, F, d_points, static_cast<const float4 *>(d_bounds),
                                      d_lambda, base, base / m, static_cast<uint32_t>(base % m), items, m, reinterpret_cast<const float2 *>(d_u),
                                      d_out, d_stacks);
            if (e != 0) return e;
        }
        return 0;
    }
    const auto kernel = model_instance(T, aim_throughput_kernel<kModelThin>, aim_throughput_kernel<kModelKolb>, aim_throughput_kernel<kModelNoLens>);
    return launch_pass(kernel, pass_grid(total), stream, T, D, F, d_points, static_cast<const float4 *>(d_bounds), d_lambda, total, m,
                       reinterpret_cast<const float2 *>(d_u), d_out);
}

}  // namespace zoic

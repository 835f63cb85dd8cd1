// spectral.hip -- camera_create_ray (RAYTRACED, zoic.cpp:1850-1964) at a wavelength per ray (spectral.hpp has the model), and with
// HERO at k wavelengths per sample: the hero's accepted try traced once more at each companion wavelength (hero.hpp has the contract).
//
// Mapping.  The launch shape of device_pass.hpp with a wave's chunk as the item; the two small passes behind the thin-lens kernel walk
// one row per lane (for_each_item).  Persistent lanes: a wave claims CHUNKS of kSpecChunk consecutive samples (grid-stride over the batch) and each lane holds
// one sample until it is finished, then takes the next sample of the chunk (ballot + mbcnt).  A round of the wave's loop is
//   * refill: free lanes take the chunk's next samples and set them up -- the reference's set-up arithmetic (setup_ray<true>: sensor
//     point, exit-pupil LUT, parabola rotation), the sample's own lens point, the ray's wavelength;
//   * candidate search: a lane whose try dies at interface 0 (a clip there is geometry only: the wavelength plays no part) draws
//     the next lens sample from its retry stream, as the pool kernels do -- tries and stream advance exactly as in the reference's
//     loop -- while enough lanes are looking (kSpecMinSearching) or no lane has a candidate yet;
//   * trace: the candidates go through every interface with the eta and TIR rule of THEIR wavelength;
//   * the finished rays' records are written and their counts kept per lane; a failed try goes back to the search.
// Dead pixels (outside the image circle, all 27 tries are one) and retry-dead rays (no retry can reach the rear element:
// dead_ray_end) end after their first try, as in the pool kernels.
// HERO adds a life to the lane: a hero that finishes with weight keeps its lane and its start (os, ds) -- saved in front of every
// trace, in STRICT as in FAST -- and goes back into the round's trace stage as a candidate at the next companion's dl, column after
// column, before the lane takes the next sample.  Hero tries and companions of different lanes run through the same trace instruction
// stream, so the trace stage stays as full as without companions; set-up, the reference sampler's gathers and the interface-0 search
// are paid once per sample, not per wavelength.  A hero of weight 0 writes its k - 1 lost records at once and frees the lane.  k is a
// wave-uniform kernel argument; no loop is unrolled over it.  Without HERO k is the constant 1 and all of this compiles away: column 0
// and the counters are one body's, whatever k.
// STRICT: trace_lens_spectral_strict (spectral.hpp), the reference's arithmetic bit for bit.  FAST (both FAST modes): f32 with
// explicit FMAs (fast_optics.hpp FastHit / fast_refract) on per-lane eta, qOffset and krScale; set-up, lens samples, directions and
// the interface-0 test stay the reference's, and a try with a clip inside a guard band (FastSurface::housingLo/Hi) is traced again
// in the reference's arithmetic from the same start: every clip decision is either a FAST one outside its band or a STRICT one.
#include <hip/hip_runtime.h>

#include "hero.hpp"
#include "record_pass.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {
namespace {

constexpr uint32_t kSpecChunk = 256;           // samples per claim of a wave: 4 per lane
constexpr uint32_t kSpecMinSearching = 16;     // the search goes on while at least this many lanes are looking

// The ray kernels' argument list (device_pass.hpp kernarg_view): the traces read the tables through the kernarg segment (spectral.hpp
// ZOIC_SPEC_PIN).  T first: kernarg_fast_surfaces() (fast_optics.hpp) counts on it.
struct SpectralKernelArgs {
    KolbTable T; SpectralTable W; BokehTables B; const float4 *samples; const float *lambdas; const uint4 *rngStates; uint64_t rayBase; uint64_t n;
    RayRecord *out; DeviceCounters *counters; uint32_t k;
};
__device__ __forceinline__ auto kernarg_surfaces() { return kernarg_view<SpectralKernelArgs, Surface>(offsetof(SpectralKernelArgs, T) + offsetof(KolbTable, surf)); }
__device__ __forceinline__ auto kernarg_spectral() { return kernarg_view<SpectralKernelArgs, SpectralTable>(offsetof(SpectralKernelArgs, W)); }

__device__ __forceinline__ bool trace_strict(int count, float dl, V3 &o, V3 &d, uint32_t &tirCount)
{
    return trace_lens_spectral_strict(kernarg_surfaces(), kernarg_spectral(), count, dl, o, d, tirCount);
}

// One trace in FAST arithmetic with the per-lane constants of the lane's wavelength.  (o, d) as trace_lens_fast_rolled leaves
// them; `unsure`: a clip decision inside its interface's guard band was met (the caller then traces the same start in STRICT).
__device__ __forceinline__ bool trace_fast(int n, float dl, V3 &o, V3 &d, uint32_t &tirCount, bool &unsure)
{
    const float inv = frsq_fast(fast_norm2(d));
    V3 u{d.x * inv, d.y * inv, d.z * inv};
    float oAxis2 = fast_axis2(o);
    bool ok = true, refracted = false;
    auto W = kernarg_spectral();
    float n1 = ffma(W->cauchyB[0], dl, W->iorD[0]);
    for (int ii = 0; ii < n; ++ii) {
        const int i = __builtin_amdgcn_readfirstlane(ii);
        FastSurface S = load_surface<true>(kernarg_fast_surfaces(), i);
        ZOIC_SPEC_PIN(W);
        const float n2 = (i + 1 < n) ? ffma(W->cauchyB[i + 1], dl, W->iorD[i + 1]) : 1.0f;
        // eta = n1 / n2 (== n1 where n2 == 1, zoic.cpp:1013); qOffset = R^2 (1 - eta^2) / eta^2 = R^2 (n2 - n1)(n2 + n1) / n1^2 (no
        // cancellation at cemented interfaces); krScale = eta / (|R| R)
        S.eta = n1 * frcp_fast(n2);
        S.qOffset = S.radius2 * (((n2 - n1) * (n2 + n1)) * frcp_fast(n1 * n1));
        S.krScale = S.eta * W->invAbsRR[i];
        bool near = false;
        const int r = fast_interface(S, o, oAxis2, u, &near);
        unsure |= near;
        if (r != 0) { if (r == 2) ++tirCount; ok = false; break; }
        refracted = true;
        n1 = n2;
    }
    if (refracted) d = u;
    return ok;
}

// the ray's private retry stream before its first draw (the pool kernels' seeding)
__device__ __forceinline__ Rng ray_stream(const uint4 *rngStates, uint32_t seed, uint64_t rayBase, uint64_t idx)
{
    if (rngStates) { const uint4 r = rngStates[idx]; return Rng{r.x, r.y, r.z, r.w}; }
    return rng_for_ray(seed, rayBase + idx);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void store_zero_record(RayRecord *out, uint64_t at, uint32_t flags)
{
    store_ray_record(out, at, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, flags);
}

// the tail of the passes behind the thin-lens kernel: the counts it gave rejected rows are taken back (`flags`: such a row's record)
__device__ __forceinline__ void count_taken_back(uint32_t flags, uint32_t &succ, uint32_t &vign)
{
    if (record_tries(flags) > static_cast<uint32_t>(kMaxTries)) ++vign; else ++succ;
}
__device__ __forceinline__ void take_back(DeviceCounters *counters, uint32_t succ, uint32_t vign)
{
    DeviceCounters *cs = counter_set(counters);
    succ = wave_sum(succ); vign = wave_sum(vign);
    if (cs && (threadIdx.x & 63u) == 0u) {   // two's complement: the host sums the counter sets modulo 2^64
        if (succ) atomicAdd(&cs->succes, 0ull - static_cast<unsigned long long>(succ));
        if (vign) atomicAdd(&cs->vignetted, 0ull - static_cast<unsigned long long>(vign));
    }
}

}  // namespace

// budget: 0 scratch, 0 spills.  HERO: k = kRows wavelengths per sample, record (idx, col) at out[idx k + col]; otherwise k is 1 and every
// hero-only statement below (col, hflags, hw, the saved start, the advance stage, the lost companions) is compiled away.
template <bool FAST, bool HERO>
__global__ __launch_bounds__(kPassBlock) void kolb_spectral_kernel(const KolbTable T, const SpectralTable W, const BokehTables B,
                                                                   const float4 *__restrict__ samples, const float *__restrict__ lambdas,
                                                                   const uint4 *__restrict__ rngStates, uint64_t rayBase, uint64_t n,
                                                                   RayRecord *__restrict__ out, DeviceCounters *counters, uint32_t kRows)
{
    const uint32_t k = HERO ? kRows : 1u;
    __shared__ __align__(16) float2 lut[kLutEntries];
    stage_lut(T, lut);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kPassBlock / 64);
    const uint64_t waveId = static_cast<uint64_t>(blockIdx.x) * (kPassBlock / 64) + (threadIdx.x >> 6);
    const uint32_t kOut = static_cast<uint32_t>(kMaxTries) + 1u;
    uint32_t succ = 0, vign = 0, tir = 0;

    for (uint64_t chunk = waveId * kSpecChunk; chunk < n; chunk += waves * kSpecChunk) {
        const uint64_t end = (n - chunk < kSpecChunk) ? n : chunk + kSpecChunk;
        uint64_t next = chunk;   // wave-uniform
        bool busy = false, searching = false, cand = false, finiteSample = true;
        uint64_t idx = 0;
        uint32_t tries = 0;
        uint32_t col = 0;        // the column this lane works on: 0 the hero's tries, j >= 1 the companion at lambdas[idx k + j]
        uint32_t hflags = 0;     // the finished hero's flags and weight: what its companions carry
        float hw = 0.0f;
        float dl = 0.0f;
        RaySetup rs{};
        Rng rng{1u, 2u, 3u, 4u};
        V3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
        V3 os = o, ds = d;       // the start of the lane's last trace: the hero's accepted try leaves its companions' start here
        for (;;) {
            // ---- refill ---------------------------------------------------------------------------------------------------
            const unsigned long long freeMask = __ballot(!busy);
            bool fresh = false;
            if (next < end && freeMask != 0ull) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(freeMask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(freeMask), 0u));
                const uint64_t left = end - next;
                if (!busy && rank < left) { idx = next + rank; fresh = true; }
                const uint64_t took = static_cast<uint64_t>(__popcll(freeMask));
                next += took < left ? took : left;
            }
            if (fresh) {
                const float lambda = lambdas[idx * k];
                if (!spectral_valid(lambda)) {   // an invalid hero rejects the whole row; no counter
#pragma nounroll
                    for (uint32_t j = 0; j < k; ++j) store_zero_record(out, idx * k + j, kSpectralRejected);
                } else {
                    busy = true;
                    col = 0u;
                    const float4 s = samples[idx];
                    dl = spectral_dl(lambda);
                    rs = setup_ray<true>(T, lut, s.x, s.y);
                    tries = 0;
                    o = V3{rs.o0x, rs.o0y, T.originShift};
                    V2 lens = lens_sample<true>(T, B, nullptr, s.z, s.w);                       // zoic.cpp:1870
                    finiteSample = (fabsf(lens.x) <= 3.0e38f) && (fabsf(lens.y) <= 3.0e38f);
                    if (!T.useLUT) {                                                             // zoic.cpp:1873-1877
                        d = V3{(lens.x * T.rearAperture) - o.x, (lens.y * T.rearAperture) - o.y, T.dirZ};
                    } else {                                                                     // zoic.cpp:1913-1924 (x only)
                        lens.x *= rs.maxScale; lens.y *= rs.maxScale;
                        lens.x += rs.translation;
                        const float rx = lens.x * rs.cs - lens.y * rs.sn, ry = lens.x * rs.sn + lens.y * rs.cs;
                        d = V3{rx - o.x, ry - o.y, T.dirZ};
                    }
                    searching = true;
                    cand = false;
                }
            }
            if (__ballot(busy) == 0ull) {
                if (next >= end) break;
                continue;
            }

            // ---- candidate search: hero tries only, a companion is a candidate already (zoic.cpp:1927-1947: a clip at interface 0
            // bumps no counter and leaves (o, d) untouched) ------------------------------------------------------------------------
            bool done = false, failed = false, advance = false;
            for (;;) {
                const uint32_t looking = static_cast<uint32_t>(__popcll(__ballot(searching)));
                if (looking == 0u || (looking < kSpecMinSearching && __ballot(cand) != 0ull)) break;
                if (searching) {
                    bool inRange;
                    bool pass = interface0_clear_strict_lean(T, o, d, inRange);
                    if (__builtin_expect(!inRange, 0)) pass = interface0_clear_strict(T, o, d);
                    if (pass) {
                        cand = true; searching = false;
                    } else if (tries == 0u && rs.dead && finiteSample) {
                        tries = kOut; searching = false; done = true; failed = true;             // all 27 tries are this one
                    } else if (tries == 0u && (rs.flags & kRetryDeadBit) != 0u) {
                        searching = false; done = true; failed = true; tries = 0xffu;            // dead_ray_end below
                    } else if (tries >= kOut) {
                        searching = false; done = true; failed = true;
                    } else {
                        if (tries == 0u) rng = ray_stream(rngStates, T.seed, rayBase, idx);
                        const float u = rng_unit(xor128(rng));   // zoic.cpp:1930
                        const float v = rng_unit(xor128(rng));
                        ++tries;
                        d = retry_direction(T, lens_sample<true>(T, B, nullptr, u, v), rs.o0x, rs.o0y, rs.maxScale, rs.translation, rs.sn, rs.cs);
                    }
                }
            }

            // ---- the candidates' traces: hero tries and companions, each lane at its own dl ---------------------------------------
            if (__ballot(cand) != 0ull && cand) {
                cand = false;
                uint32_t tirTry = 0;
                bool ok;
                os = o; ds = d;
                if constexpr (FAST) {
                    bool unsure = false;
                    ok = trace_fast(T.lensCount, dl, o, d, tirTry, unsure);
                    if (unsure) {   // a clip too close to call: this start in the reference's arithmetic
                        o = os; d = ds; tirTry = 0;
                        ok = trace_strict(T.lensCount, dl, o, d, tirTry);
                    }
                } else {
                    ok = trace_strict(T.lensCount, dl, o, d, tirTry);
                }
                if (HERO && col != 0u) {   // a companion: one trace, no retry, no counter
                    if (ok) store_ray_record(out, idx * k + col, o.x * -1.0f, o.y * -1.0f, o.z * -1.0f, d.x * -1.0f, d.y * -1.0f, d.z * -1.0f, hw, hflags);
                    else store_zero_record(out, idx * k + col, hflags | kHeroCompanionLost);
                    ++col;
                    advance = true;
                } else {
                    tir += tirTry;
                    if (ok) {
                        done = true;
                        failed = tries > static_cast<uint32_t>(kMaxTries);   // a success at try 26 is still out of tries (zoic.cpp:1927, 1951)
                    } else if (tries == 0u && (rs.flags & kRetryDeadBit) != 0u) {
                        done = true; failed = true; tries = 0xffu;
                    } else if (tries >= kOut) {
                        done = true; failed = true;   // the partial state of try 26 (zoic.cpp:1951-1961)
                    } else {
                        o = V3{rs.o0x, rs.o0y, T.originShift};
                        searching = true;
                        if (tries == 0u) rng = ray_stream(rngStates, T.seed, rayBase, idx);
                        const float u = rng_unit(xor128(rng));
                        const float v = rng_unit(xor128(rng));
                        ++tries;
                        d = retry_direction(T, lens_sample<true>(T, B, nullptr, u, v), rs.o0x, rs.o0y, rs.maxScale, rs.translation, rs.sn, rs.cs);
                    }
                }
            }

            // ---- finished heroes ---------------------------------------------------------------------------------------------
            if (done) {
                float w;
                uint32_t flags;
                const bool retryDead = tries == 0xffu;
                if (retryDead) {   // retries 1 ... 26 die at interface 0 (the arithmetic of the pool kernels)
                    const DeadRayEnd e = dead_ray_end<true>(T, B, nullptr, rs, ray_stream(rngStates, T.seed, rayBase, idx));
                    o = e.o; d = e.d; w = e.w;
                    flags = 1u | (e.tries << 1) | ((rs.flags & 1u) << 6);
                    if (e.nanDraw) ++succ; else ++vign;
                } else {
                    w = failed ? 0.0f : 1.0f;
                    if (T.exposureOn) w *= T.exposureMul;                                        // zoic.cpp:1981-1987
                    flags = (tries > 0u ? 1u : 0u) | (tries << 1) | ((rs.flags & 1u) << 6);
                    if (failed) ++vign; else ++succ;                                             // zoic.cpp:1951-1957
                }
                store_ray_record(out, idx * k, o.x * -1.0f, o.y * -1.0f, o.z * -1.0f, d.x * -1.0f, d.y * -1.0f, d.z * -1.0f, w, flags);   // zoic.cpp:1960-1961
                searching = false; cand = false;
                if (HERO && w != 0.0f && !retryDead) {   // the lane stays: its companions start where the accepted try started
                    hw = w; hflags = flags; col = 1u;
                    advance = true;
                } else {   // no start to share (weight 0, or a retry-dead ray's NaN draw, hero.hpp): the companions are lost; an invalid wavelength is still rejected
#pragma nounroll
                    for (uint32_t j = 1; j < k; ++j)
                        store_zero_record(out, idx * k + j, spectral_valid(lambdas[idx * k + j]) ? (flags | kHeroCompanionLost) : kSpectralRejected);
                    busy = false;
                }
            }

            // ---- the lane's next companion: invalid wavelengths are rejected on the way, after the last column the lane is free ------
            if (HERO && advance) {
                float lambda = 0.0f;
#pragma nounroll
                while (col < k) {
                    lambda = lambdas[idx * k + col];
                    if (spectral_valid(lambda)) break;
                    store_zero_record(out, idx * k + col, kSpectralRejected);
                    ++col;
                }
                if (col < k) {
                    dl = spectral_dl(lambda);
                    o = os; d = ds;
                    cand = true;
                } else {
                    busy = false;
                }
            }
        }
    }
    DeviceCounters *cs = counter_set(counters);
    succ = wave_sum(succ); vign = wave_sum(vign); tir = wave_sum(tir);
    if (cs && lane == 0u) {
        if (succ) atomicAdd(&cs->succes, static_cast<unsigned long long>(succ));
        if (vign) atomicAdd(&cs->vignetted, static_cast<unsigned long long>(vign));
        if (tir) atomicAdd(&cs->tir, static_cast<unsigned long long>(tir));
    }
}

// rows of the other lens models: invalid wavelengths -> a rejected record; the thin-lens kernel's count of that row is taken back
__global__ __launch_bounds__(kPassBlock) void spectral_reject_kernel(const float *__restrict__ lambdas, uint64_t n, RayRecord *__restrict__ out,
                                                                     DeviceCounters *counters, int countsRays)
{
    uint32_t succ = 0, vign = 0;
    for_each_item(n, [&](uint64_t i) {
        if (spectral_valid(lambdas[i])) return;
        const uint32_t flags = out[i].flags;
        if (countsRays) count_taken_back(flags, succ, vign);
        store_zero_record(out, i, kSpectralRejected);
    });
    take_back(counters, succ, vign);
}

// the same rows at k wavelengths: record i of the thin-lens kernel into the valid columns of row i, the others rejected; the count
// of a row whose hero is rejected is taken back.  (Not the pass above at k = 1: that one works in place and writes rejected rows only.)
__global__ __launch_bounds__(kPassBlock) void hero_replicate_kernel(const RayRecord *__restrict__ staged, const float *__restrict__ lambdas, uint64_t n,
                                                                    uint32_t k, RayRecord *__restrict__ out, DeviceCounters *counters, int countsRays)
{
    uint32_t succ = 0, vign = 0;
    for_each_item(n, [&](uint64_t i) {
        const float4 *p = reinterpret_cast<const float4 *>(staged + i);
        const float4 a = p[0], b = p[1];
        const uint32_t flags = __builtin_bit_cast(uint32_t, b.w);
        const bool hero = spectral_valid(lambdas[i * k]);
        if (!hero && countsRays) count_taken_back(flags, succ, vign);
#pragma nounroll
        for (uint32_t j = 0; j < k; ++j) {
            if (hero && spectral_valid(lambdas[i * k + j])) store_ray_record(out, i * k + j, a.x, a.y, a.z, a.w, b.x, b.y, b.z, flags);
            else store_zero_record(out, i * k + j, kSpectralRejected);
        }
    });
    take_back(counters, succ, vign);
}

namespace {
// k == 1: one wavelength per sample, the kernel without the hero's stages
int launch_wavelength_rays(const KolbTable &table, const SpectralTable &spec, const BokehTables &bokeh, const float *d_samples,
                           const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k, RayRecord *out,
                           DeviceCounters *d_counters, int mode, void *stream)
{
    if (n == 0) return 0;
    const auto kernel = k == 1u ? (mode == 0 ? kolb_spectral_kernel<false, false> : kolb_spectral_kernel<true, false>)
                                : (mode == 0 ? kolb_spectral_kernel<false, true> : kolb_spectral_kernel<true, true>);
    return launch_pass(kernel, pass_grid(n, static_cast<uint64_t>(kSpecChunk) * (kPassBlock / 64)), stream, table, spec, bokeh,
                       reinterpret_cast<const float4 *>(d_samples), d_lambda, reinterpret_cast<const uint4 *>(d_rng), rayBase, n, out, d_counters, k);
}
}  // namespace

int launch_kolb_spectral(const KolbTable &table, const SpectralTable &spec, const BokehTables &bokeh, const float *d_samples,
                         const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, RayRecord *out,
                         DeviceCounters *d_counters, int mode, void *stream)
{
    return launch_wavelength_rays(table, spec, bokeh, d_samples, d_lambda, d_rng, rayBase, n, 1u, out, d_counters, mode, stream);
}

int launch_kolb_hero(const KolbTable &table, const SpectralTable &spec, const BokehTables &bokeh, const float *d_samples,
                     const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k, RayRecord *out,
                     DeviceCounters *d_counters, int mode, void *stream)
{
    if (n == 0) return 0;
    if (k < 2 || k > kHeroMaxWavelengths) return static_cast<int>(hipErrorInvalidValue);   // k = 1 is launch_kolb_spectral
    return launch_wavelength_rays(table, spec, bokeh, d_samples, d_lambda, d_rng, rayBase, n, k, out, d_counters, mode, stream);
}

int launch_spectral_reject(const float *d_lambda, uint64_t n, RayRecord *out, DeviceCounters *d_counters, bool countsRays, void *stream)
{
    if (n == 0) return 0;
    return launch_pass(spectral_reject_kernel, pass_grid(n), stream, d_lambda, n, out, d_counters, countsRays ? 1 : 0);
}

int launch_hero_replicate(const RayRecord *staged, const float *d_lambda, uint64_t n, uint32_t k, RayRecord *out, DeviceCounters *d_counters,
                          bool countsRays, void *stream)
{
    if (n == 0) return 0;
    if (k < 2 || k > kHeroMaxWavelengths) return static_cast<int>(hipErrorInvalidValue);   // k = 1 is launch_spectral_reject
    return launch_pass(hero_replicate_kernel, pass_grid(n), stream, staged, d_lambda, n, k, out, d_counters, countsRays ? 1 : 0);
}

}  // namespace zoic

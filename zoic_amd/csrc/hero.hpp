// hero.hpp -- hero-wavelength rays (zoic_create_rays_hero_device): k wavelengths through ONE lens point per camera sample.
//
// A spectral renderer carries a hero wavelength and a few companions per sample.  k calls of zoic_create_rays_spectral_device run k
// retry loops: where a try passes at one wavelength and is clipped or totally reflected at another, the colours of one sample leave
// through different lens points and decorrelate into colour noise.  Here the retry loop runs once, at the hero's wavelength
// (column 0), and its accepted try fixes the start -- the sensor point and the lens point after the exit-pupil transform, the
// (o, d) the hero's trace began with.  Every companion (column j >= 1) is that same start traced once through every interface with
// the indices of its own wavelength (spectral.hpp: the model, the validity range, the STRICT trace):
//   * it comes through: origin and direction after the final flip, the hero's weight, the hero's flags;
//   * it misses a sphere, is clipped at a housing or the stop, or is totally reflected: origin = dir = +0.0, weight 0, the hero's
//     flags | kHeroCompanionLost.  No retry is drawn for it: that is where a fringe ends.
// A hero of weight 0 (out of tries, a dead pixel, retry-dead) has no start: its companions are lost records.  So are those of the one
// hero that has weight without an accepted try: a retry-dead ray one of whose draws lands on the disk's centre (probability 2e-15 per
// draw; kolb_pool_body.hpp dead_ray_end reproduces the reference's NaN ray of weight 1 there) -- a NaN ray is no start.  Companions touch no
// counter and advance no retry stream.  A companion whose wavelength is invalid is rejected alone (kSpectralRejected); an invalid
// hero rejects the whole row.  The hero's record and the counters are the spectral call's, bit for bit; a companion at the hero's
// own wavelength repeats the hero's trace operation for operation and so its record.
//
// Records are sample-major: record (i, j) at out[i * k + j], 2 <= k <= kHeroMaxWavelengths in the launchers below (the entry point hands k = 1
// to the spectral call).
#pragma once
#include <cstdint>

#include "spectral.hpp"

namespace zoic {

constexpr uint32_t kHeroMaxWavelengths = 8;
constexpr uint32_t kHeroCompanionLost = 0x100u;   // flag bit 8: the companion did not come through at the hero's lens point

// ---- launchers (spectral.hip) ------------------------------------------------------------------------------------------
// RAYTRACED: d_lambda = n x k f32 (nm), hero first; out = n x k records.  mode as launch_kolb_spectral.  Ray i draws from the stream
// keyed by rayBase + i (or d_rng[i]); the counters move as launch_kolb_spectral's on column 0.
int launch_kolb_hero(const KolbTable &table, const SpectralTable &spec, const BokehTables &bokeh, const float *d_samples,
                     const float *d_lambda, const uint32_t *d_rng, uint64_t rayBase, uint64_t n, uint32_t k, RayRecord *out,
                     DeviceCounters *d_counters, int mode, void *stream);
// The other lens models ignore the wavelength: `staged` holds the n records of launch_thin_rays; this pass copies record i into the
// valid columns of row i, rejects the invalid ones (the whole row where the hero's wavelength is invalid) and takes back the counter
// bump the thin-lens kernel gave a rejected hero (countsRays as launch_spectral_reject).  The staging buffer is the camera's (capi.cpp
// HeroStage): one per camera, so THINLENS hero calls of one camera run one after the other on the device.
int launch_hero_replicate(const RayRecord *staged, const float *d_lambda, uint64_t n, uint32_t k, RayRecord *out, DeviceCounters *d_counters,
                          bool countsRays, void *stream);

}  // namespace zoic

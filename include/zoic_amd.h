/*
 * include/zoic_amd.h -- C-ABI of libzoic_amd.so, the MI355X (gfx950) camera-ray generator for
 * zoic's per-sample lens hot path.
 *
 * Drop-in boundary.  zoic is an Arnold camera node: Arnold calls the method table
 * (AI_CAMERA_NODE_EXPORT_METHODS(zoicMethods), zoic.cpp:61; returned by NodeLoader,
 * zoic.cpp:1999-2007) -- node_parameters / node_initialize / node_update / node_finish /
 * camera_create_ray.  Each entry point below replaces one of those methods (file:line cited
 * per function) with plain pointers and sizes; no C++ or torch types cross this boundary.
 * INTEGRATION.md shows the binding a zoic maintainer would add inside zoic.cpp.
 *
 * All compute entry points run hand-written HIP kernels; there is no CPU fallback.  Every
 * function returns a zoic_status; ZOIC_OK == 0.
 *
 * Threading contract -- the reference's own (Arnold calls node_initialize / node_update / node_finish from one
 * thread with no sample in flight, and camera_create_ray concurrently from every render thread, zoic.cpp:1752):
 *   - zoic_camera_create / _update / _destroy / _set_* / _reset_counters: one thread at a time per camera, and no
 *     ray call of that camera running on another thread.  (_update and _destroy wait for launches still queued.)
 *   - zoic_create_rays_device / _host / _arnold / _arnold_differentials / _device_resident, zoic_ray_differentials_device, zoic_ray_differentials_spectral_device, zoic_create_rays_hero_device, zoic_create_ghost_rays_device, zoic_camera_create_ray, zoic_camera_create_rays_tile, zoic_tile_submit / _wait /
 *     _done (one tile per thread), zoic_camera_reverse_ray, zoic_project_points_device, zoic_project_point, zoic_trace_back_rays_device, zoic_trace_back_ray, zoic_trace_back_jacobian_device, zoic_trace_back_ray_jacobian, zoic_pupil_bounds_device, zoic_pupil_bounds_point, zoic_splat_points_device, zoic_splat_point (and their _spectral forms), zoic_camera_get_counters, zoic_camera_set_wait_mode: any number of host threads on one camera at once.  Each call works on private
 *     scratch and private HIP streams and waits only for its own work; results do not depend on the interleaving
 *     (batched calls key every ray's retry stream by its global ray index, the per-sample call by its tid).
 *   - No entry point changes the calling thread's current HIP device.
 */
#ifndef ZOIC_AMD_H
#define ZOIC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (a plug-in shim checks zoic_abi_version() == ZOIC_AMD_ABI_VERSION at load and refuses anything else):
 *   1  round 1.
 *   2  round 2: zoic_create_rays_arnold, zoic_host_*, per-tid retry streams.
 *   3  round 3/4: zoic_lens_info gained the trailing fastRunsStrict (zoic_camera_get_info writes sizeof(zoic_lens_info) bytes:
 *      a v2 caller's struct is 8 bytes short, see the end of this entry); zoic_create_rays_arnold WRITES EVERY OUTPUT ROW WHOLE (v2 updated fields in
 *      place); zoic_camera_create_ray runs through a resident kernel, so a caller's hipDeviceSynchronize / hipFree can wait up
 *      to 50 ms for it to retire (zoic_camera_get_counters / _update / _destroy stop it first); the zoic_frame_* entry points
 *      (one frame over several devices of this process); zoic_lens_info gained precomputeTIR behind fastRunsStrict (8 bytes in all).
 *   4  round 5: zoic_tile_* / zoic_camera_create_rays_tile (bucket-sized batches through the resident kernel, no launch);
 *      zoic_frame_get_lane_info; ZOIC_FRAME_PAYLOAD_SPARSE; zoic_camera_set_frame_aspect; zoic_tile_set_rows / zoic_tile_rays, zoic_tile_set_inputs / zoic_tile_samples.
 *      Nothing of ABI 3 changed shape.
 *   5  round 6: zoic_camera_set_wait_mode (how a render thread waits for the resident kernel: spin / yield / sleep); a zoic_tile that
 *      outlives its camera is DETACHED by zoic_camera_destroy (every call but zoic_tile_destroy fails, the array getters return NULL)
 *      instead of dangling; zoic_tile_done restarts a resident kernel that retired under the poll; ZOIC_FRAME_PAYLOAD_AUTO +
 *      zoic_frame_auto_layout (the gather's layout chosen from the camera's dead-ray fraction); zoic_create_rays_device_resident (device
 *      buffers through the resident kernel, no launch).  Nothing of ABI 4 changed shape.
 *      Added later without a new number (additive: nothing existing changed shape or behaviour): zoic_ray_differential,
 *      zoic_ray_differentials_device and zoic_create_rays_arnold_differentials (traced ray differentials).
 *      Added later without a new number (additive): zoic_create_rays_spectral_device, zoic_camera_get_dispersion and
 *      zoic_camera_set_abbe_numbers (rays at a wavelength per ray: chromatic aberration); flag bit 7 of zoic_ray (wavelength rejected).
 *      Added later without a new number (additive): zoic_project_points_device, zoic_project_point and
 *      zoic_camera_set_reverse_projection (reverse projection; zoic_camera_reverse_ray answers only when opted in).
 *      Added later without a new number (additive): zoic_trace_back_rays_device and zoic_trace_back_ray (trace-back: camera rays
 *      to the screen samples they land on).
 *      Added later without a new number (additive): zoic_ray_differentials_spectral_device (traced ray differentials of spectral
 *      records, with the derivative with respect to the wavelength).
 *      Added later without a new number (additive): zoic_create_rays_hero_device (k wavelengths through one lens point per sample),
 *      ZOIC_HERO_MAX_WAVELENGTHS; flag bit 8 of zoic_ray (ZOIC_RAY_COMPANION_LOST).
 *      Added later without a new number (additive): zoic_trace_back_jacobian_device, zoic_trace_back_ray_jacobian and their
 *      _spectral forms (the trace-back with its Jacobian dPs / d(origin, dir)).
 *      Added later without a new number (additive): zoic_ray_transmittance_device, zoic_camera_set_coatings and
 *      zoic_camera_get_coatings (the Fresnel transmittance of traced rays, with single-layer coatings).
 *      Added later without a new number (additive): zoic_camera_set_coating_stacks, zoic_camera_get_coating_stacks and
 *      ZOIC_COATING_MAX_LAYERS (multilayer coatings: thin-film stacks for the transmittance calls and the ghosts' weights).
 *      Added later without a new number (additive): zoic_create_ghost_rays_device and zoic_camera_get_ghost_pairs (ghost rays: the
 *      two-reflection paths through the lens with their Fresnel weights), ZOIC_GHOST_MAX_PAIRS and the ZOIC_GHOST_* flag macros.
 *      Added later without a new number (additive): zoic_pupil_bounds_device, zoic_pupil_bounds_point and their _spectral forms
 *      (pupil bounds: the lens area a scene point sees and the box of its blur spot), zoic_pupil_bounds and the ZOIC_PUPIL_* macros.
 *      Added later without a new number (additive): zoic_splat_points_device, zoic_splat_point and their _spectral forms (lens splats:
 *      scene points through drawn aims in their pupil boxes to the screen, with two measures), zoic_splat and ZOIC_SPLAT_NO_BOX. */
#define ZOIC_AMD_ABI_VERSION 5

typedef enum zoic_status {
    ZOIC_OK = 0,
    ZOIC_ERR_INVALID_ARGUMENT = 1,
    ZOIC_ERR_LENS_PATH = 2,        /* "[ZOIC] Lens Data Path is invalid"            zoic.cpp:1639-1642 */
    ZOIC_ERR_LENS_COLUMNS = 3,     /* "<4 / >5 columns of data"                     zoic.cpp:745-754   */
    ZOIC_ERR_LENS_PARSE = 4,       /* std::stof would throw                         zoic.cpp:774 ff.   */
    ZOIC_ERR_MULTI_APERTURE = 5,   /* "Multiple apertures found"                    zoic.cpp:926-929   */
    ZOIC_ERR_NO_APERTURE = 6,      /* no zero-radius row: apertureElement would be read uninitialised (zoic.cpp:922,1115,1668) */
    ZOIC_ERR_TOO_MANY_LENSES = 7,  /* > ZOIC_MAX_LENS_SURFACES rows */
    ZOIC_ERR_BOKEH_IMAGE = 8,      /* "[ZOIC] Couldn't open bokeh image!"           zoic.cpp:1589-1592 */
    ZOIC_ERR_NOT_UPDATED = 9,      /* create_rays before a successful update */
    ZOIC_ERR_HIP = 10,             /* HIP runtime error; zoic_last_error_string() has the text */
    ZOIC_ERR_NO_DEVICE = 11        /* no gfx950 device visible: this library has no CPU path */
} zoic_status;

/* enum LensModel, zoic.cpp:84-88 */
typedef enum zoic_lens_model { ZOIC_THINLENS = 0, ZOIC_RAYTRACED = 1, ZOIC_LENS_NONE = 2 } zoic_lens_model;

/* arithmetic mode of the kernels */
typedef enum zoic_precision {
    ZOIC_PRECISION_STRICT = 0, /* the reference's operation order, no FMA contraction, its f64 intermediates: bit-exact vs the CPU oracle */
    ZOIC_PRECISION_FAST = 1,   /* same algorithm, f32 only, FMA/rsq, redundant normalisations removed: direction RMSE < 1e-5.
                                  Decision-safe: housing / stop clips that lie inside the interface's guard band (wide at the stop,
                                  which the reference traces as a sphere of |R| ~ 1e4 cm; a few ulps elsewhere), and the
                                  exit-pupil LUT's edge, are re-taken in STRICT arithmetic (a second kernel over the few rays
                                  concerned).  Sphere-miss and TIR decisions are not guarded: residual flips of try count /
                                  weight: none in 33.5 M rays of each benchmark configuration (tests hold 5e-5); origin / direction
                                  differ in low-order bits */
    ZOIC_PRECISION_FAST_UNCHECKED = 2 /* FAST without the decision check (A/B; decisions flip where the reference's own f32
                                         rounding noise decides, ~1e-5 ... 1e-3 of the rays depending on the lens) */
    /* Domain of the FAST modes: they drop the reference's per-interface renormalisations (the refracted direction stays unit
       by construction as long as every hit lies ON its sphere to rounding), which holds while hits are the near-vertex roots
       of a lens laid out rear -> front with the sensor behind it.  A prescription whose traced focal length is negative is
       rescaled by a NEGATIVE focalLengthRatio (zoic.cpp:1651-1661: thicknesses and radii change sign), and one whose focus
       computation puts the sensor in FRONT of the rear vertex (originShift >= lenses[0].thickness) sends its rays away from
       the lens: the reference's one signed root (zoic.cpp:986, t < 0 never rejected) then lands far behind the ray, and the
       hit-point rounding no longer is small against the radii.  Such a camera (zoic_lens_info::fastRunsStrict) runs STRICT in
       every mode.  So does a camera that fails zoic_camera_update's self-check: TWO slabs of 4096 probe samples each (two jitters
       of a 64 x 64 lattice over sx in [-1, 1], sy in [-a, a], a = zoic_camera_set_frame_aspect's value, 1.0 by default) go through
       the STRICT and the decision-safe FAST kernels, and the FAST modes are kept only if, on EACH slab, at most one ray is decided
       differently and the direction RMSE of the others is < 5e-6 -- half of the 1e-5 tolerance (0.3 ms per update that rebuilds
       tables; no counter, no retry stream is touched; a HIP failure inside the check is an error of the update). */
} zoic_precision;

#define ZOIC_MAX_LENS_SURFACES 32
#define ZOIC_DEVICE_NONE (-1) /* zoic_camera_create: tables-only camera (host precompute of node_update; cannot make rays) */
#define ZOIC_LUT_ENTRIES 32 /* exitPupilLUT(&ld, 32, 100000), zoic.cpp:1692 */

/* The 14 node parameters: names, types and defaults of node_parameters (zoic.cpp:1547-1562),
 * read by cameraParams::fromNode (zoic.cpp:578-593). */
typedef struct zoic_params {
    float sensorWidth;               /* 3.6  cm */
    float sensorHeight;              /* 2.4  cm */
    float focalLength;               /* 2.0  cm */
    float fStop;                     /* 4.0     */
    float focalDistance;             /* 100  cm */
    int32_t useImage;                /* false   */
    const char *bokehPath;           /* ""  : identity of the bokeh image (change detection, zoic.cpp:608-611);
                                              a ".pfm" path is loaded from disk unless pixels were supplied by
                                              zoic_camera_set_bokeh_image */
    int32_t lensModel;               /* RAYTRACED */
    const char *lensDataPath;        /* ""  : tabular .dat lens prescription */
    int32_t kolbSamplingLUT;         /* true    */
    int32_t useDof;                  /* true    */
    float opticalVignettingDistance; /* 0.0     */
    float opticalVignettingRadius;   /* 1.0     */
    float exposureControl;           /* 0.0     */
} zoic_params;

/* AtCameraInput / AtCameraOutput (Arnold 5 ai_cameras.h) as PODs; zoic reads
 * input.{sx,sy,lensx,lensy} and writes output.{origin,dir,weight,dOdy,dDdy} (zoic.cpp:1752-1990). */
typedef struct zoic_camera_input { float sx, sy, dsx, dsy, lensx, lensy, relative_time; } zoic_camera_input;
typedef struct zoic_vec3 { float x, y, z; } zoic_vec3;
typedef struct zoic_camera_output {
    zoic_vec3 origin, dir, dOdx, dOdy, dDdx, dDdy;
    float weight[3];
} zoic_camera_output;

/* Batch output: one 32-byte record per ray (the fields of AtCameraOutput that zoic writes, zoic.cpp:1752-1990).
 * flags: bit0 = retried (tries > 0  => the caller sets dOdy=origin, dDdy=dir, zoic.cpp:1974-1977),
 *        bits1-5 = tries (0..26; 26 => weight 0, zoic.cpp:1951-1953), bit6 = outside the exit-pupil LUT (fenced UB),
 *        bit7 = wavelength rejected (zoic_create_rays_spectral_device: the record is all zero but for flags == 0x80),
 *        bit8 = companion lost (zoic_create_rays_hero_device only: ZOIC_RAY_COMPANION_LOST). */
typedef struct zoic_ray {
    float ox, oy, oz;   /* output.origin */
    float dx, dy, dz;   /* output.dir    */
    float weight;       /* output.weight (r == g == b; the caller's initial weight is taken as 1) */
    uint32_t flags;
} zoic_ray;

/* struct cameraData (zoic.cpp:627-643) + its device tables */
typedef struct zoic_camera zoic_camera;
/* succesRays / vignettedRays / totalInternalReflection of struct Lensdata (zoic.cpp:533-534), printed by node_finish */
typedef struct zoic_counters { uint64_t succesRays, vignettedRays, totalInternalReflection; } zoic_counters;

/* ---- environment ---------------------------------------------------------------------------
 * The library reads three environment variables, all of them about WHERE node_update builds its tables (the tables are
 * identical either way; tests/test_parity_gpu.py compares both builds).  None selects a CPU ray path: there is none.
 *   ZOIC_LUT_HOST=1    exit-pupil LUT (draws, probe traces, bounding boxes) built by the host loop instead of lut_build.hip;
 *                      =2: probes traced on the GPU, draws and the order-dependent box replay on the host (round 1's build)
 *   ZOIC_CDF_HOST=1    bokeh CDFs (bokehProbability) built by the host loop instead of bokeh_cdf.hip
 *   ZOIC_CELLS_HOST=1  bokeh cell records built by the host loop instead of build_cells_kernel
 * Kernel tuning constants are compile-time (-D, tools/build_variant.sh): ZOIC_MIN_SEARCHING, ZOIC_CHUNK_RAYS, ZOIC_GRID_BLOCKS,
 * ZOIC_GUARD_SCALE, ZOIC_RETRY_DEAD_MIN_SHARE. */

/* ---- library ------------------------------------------------------------------------------- */
int         zoic_abi_version(void);
const char *zoic_status_string(zoic_status);
const char *zoic_last_error_string(void);          /* thread-local detail of the last failure */
int         zoic_device_count(void);               /* gfx950 devices visible to HIP */
/* NUMA node of the host the device hangs off (sysfs, via its PCI bus id), -1 if unknown: render threads that call
 * zoic_camera_create_ray save ~1 us per call when they run on that node */
int         zoic_device_numa_node(int device);

/* ---- node lifetime ------------------------------------------------------------------------- */
/* node_parameters defaults, zoic.cpp:1547-1562 */
void zoic_params_default(zoic_params *p);
/* node_initialize, zoic.cpp:1565-1572 (`new cameraData()`); binds the camera to one HIP device.
 * device == ZOIC_DEVICE_NONE gives a tables-only camera: update() runs the host precompute (lens parse, focus,
 * exit-pupil LUT, bokeh CDF) and the get_info/get_bokeh_tables getters work, but every create_rays call fails
 * with ZOIC_ERR_NO_DEVICE -- there is no CPU ray path. */
zoic_status zoic_camera_create(int device, zoic_camera **out);
/* node_finish, zoic.cpp:1723-1749 (`delete camera`) */
void zoic_camera_destroy(zoic_camera *cam);
/* node_update, zoic.cpp:1575-1720: bokeh CDF build, lens parse + precompute + exit-pupil LUT, upload */
zoic_status zoic_camera_update(zoic_camera *cam, const zoic_params *p);
/* replaces AiTextureGetResolution / AiTextureGetNumChannels / AiTextureLoad (zoic.cpp:101-103,176-186):
 * the pixels (row-major, nchannels interleaved floats) the next update uses when useImage is set */
zoic_status zoic_camera_set_bokeh_image(zoic_camera *cam, int width, int height, int nchannels, const float *pixels);
/* lens prescription text in memory instead of fopen(lensDataPath) (readTabularLensData, zoic.cpp:708-914) */
zoic_status zoic_camera_set_lens_text(zoic_camera *cam, const char *text, size_t len);
zoic_status zoic_camera_set_precision(zoic_camera *cam, zoic_precision mode);
/* The largest |sy| the renderer will send (Arnold's convention: sx in [-1, 1], sy in [-1/aspect, 1/aspect]): the extent
 * of the frame zoic_camera_update's self-check of the FAST modes spreads its probe samples over.  Default 1.0 (a square frame; a
 * 3:2 frame is inside it); a portrait frame passes its own 1/aspect > 1.  Takes effect at the next update that rebuilds tables
 * (or at once for the verdict of the next update when the value changed). */
zoic_status zoic_camera_set_frame_aspect(zoic_camera *cam, float max_abs_sy);
/* How a render thread waits for the camera's RESIDENT kernel (zoic_camera_create_ray, zoic_tile_wait, zoic_camera_create_rays_tile).
 *   ZOIC_WAIT_SPIN   (default) a `pause` loop on the reply / the tile's flags: lowest latency, one core per waiting thread.  Right when
 *                    the render threads have a core each.
 *   ZOIC_WAIT_YIELD  spins for ~2 us, then sched_yield() between polls: for hosts with more render threads than CORES.  (Under a CPU quota
 *                    with idle cores -- a container -- sched_yield returns at once and burns quota like the spin: use ZOIC_WAIT_SLEEP there.)
 *   ZOIC_WAIT_SLEEP  spins for ~2 us, then sleeps 20 us between polls: a waiting thread costs next to nothing; +10-20 us per call.
 *                    [MI355X box, 16-CPU quota, 4096-sample tiles] 64 threads: 573 Mrays/s, p99 0.58 ms (spinning: 240 Mrays/s, p99 10 ms;
 *                    16 threads spinning: 490); 128 threads: 575 Mrays/s (profiles/ab_r06/tile_threads_wait_modes.txt).
 * Any thread, any time; takes effect at the next wait. */
typedef enum zoic_wait_mode { ZOIC_WAIT_SPIN = 0, ZOIC_WAIT_YIELD = 1, ZOIC_WAIT_SLEEP = 2 } zoic_wait_mode;
zoic_status zoic_camera_set_wait_mode(zoic_camera *cam, zoic_wait_mode mode);
/* seed of the per-ray retry streams (see zoic_create_rays_device) */
zoic_status zoic_camera_set_seed(zoic_camera *cam, uint32_t seed);

/* ---- the hot path: camera_create_ray, zoic.cpp:1752-1990 ----------------------------------- */
/* n samples already resident in device memory.
 *   d_samples    : n x (sx, sy, lensx, lensy) f32, 16-byte aligned (AtCameraInput fields zoic reads)
 *   d_rng_states : NULL, or n x 4 u32 xorshift128 states (zoic.cpp:647-652), one private retry stream per ray.
 *                  NULL => ray i uses the stream seeded from (seed, ray_index_base + i), so results do not
 *                  depend on how the image is split over launches or GPUs.
 *   d_rays       : n zoic_ray records in device memory, 16-byte aligned
 *   stream       : hipStream_t (NULL = default stream).  Asynchronous.
 * The reference draws retries from ONE process-global stream shared (racily) by all render threads
 * (zoic.cpp:648); a per-ray stream is the only order-independent restatement. */
zoic_status zoic_create_rays_device(zoic_camera *cam, uint64_t n, const float *d_samples, const uint32_t *d_rng_states,
                                    uint64_t ray_index_base, zoic_ray *d_rays, void *stream);
/* same, host buffers: H2D, kernels, D2H in pieces on three private streams (copy-in, kernels, copy-out); returns when h_rays is complete */
zoic_status zoic_create_rays_host(zoic_camera *cam, uint64_t n, const float *h_samples, const uint32_t *h_rng_states,
                                  uint64_t ray_index_base, zoic_ray *h_rays);
/* Arnold-layout batch: n AtCameraInput -> n AtCameraOutput (host arrays; page-locked ones -- zoic_host_alloc /
 * zoic_host_register -- move at PCIe rate).  Every output row is WRITTEN WHOLE (the expansion runs on the GPU): origin, dir,
 * weight[3] = the exposure factor or 0 (the caller's initial weight is taken as 1), dOdy = origin and dDdy = dir for rays
 * that retried (zoic.cpp:1974-1977), and 0 in what camera_create_ray leaves alone (dOdx, dDdx; dOdy, dDdy of first-try
 * rays) -- the values of a zero-initialised AtCameraOutput.  The thin-lens branch reads output.origin (zoic.cpp:1777): it is
 * taken as 0, as Arnold hands it in.  Ray i draws its retries from the stream keyed by ray_index_base + i. */
zoic_status zoic_create_rays_arnold(zoic_camera *cam, uint64_t n, const zoic_camera_input *inputs,
                                    zoic_camera_output *outputs, uint64_t ray_index_base);

/* ---- traced ray differentials (opt-in; csrc/differentials.hpp has the full definition) ------------------------------------
 * The ray entry points above keep the reference's derivative fields (zoic.cpp:1971-1977: dOdx = dDdx = 0, dOdy = origin and
 * dDdy = dir for retried rays), which are not derivatives.  These two calls compute them.  For a ray with weight > 0 and
 * (sx, sy) its screen sample:
 *   RAYTRACED  the accepted try (tries = bits 1-5 of the flags) starts at the sensor point o = (sx sw/2, sy sw/2, originShift),
 *              sw = sensorWidth, and aims at the lens point L -- the try's sample after the exit-pupil transform (with the LUT:
 *              scale, translation, rotation, zoic.cpp:1891-1943; without it the sample times lenses[0].aperture).  The derivatives
 *              hold L FIXED while (sx, sy) move o, and follow the ray through every interface and the final flip (zoic.cpp:1959).
 *   THINLENS   the lens point (the origin) is held fixed: dO = 0, dD = d/ds normalize(p |focalDistance| - origin) with the z flip,
 *              p = (sx tan_fov, sy tan_fov, 1); without DOF d/ds normalize(p).
 *   dOdx = dO/dsx * dsx, dOdy = dO/dsy * dsy, likewise for D (Arnold's convention).  Rays of weight 0 (the exhausted ones
 *   included) and every ray of lensModel NONE get +0.0 in all 12 floats.  Rays outside the exit-pupil LUT (flag bit 6) are
 *   differentiated through the same fenced lookup the ray kernels used.
 * The result is the derivative of the path the record took (not a finite difference; the unit-square sample is not held fixed).
 * The arithmetic is the same in every precision mode: STRICT and FAST cameras give bitwise-equal differentials on rays whose
 * tries agree.  Not covered (their derivative fields stay the reference's): zoic_camera_create_ray and the tiles (resident
 * kernel), zoic_create_rays_host, zoic_frame_*.  The records of zoic_create_rays_spectral_device have a call of their own:
 * zoic_ray_differentials_spectral_device, below. */
typedef struct zoic_ray_differential { zoic_vec3 dOdx, dOdy, dDdx, dDdy; } zoic_ray_differential;   /* 48 bytes */
/* The differentials of rays zoic_create_rays_device made: pass what that call was given (d_samples, d_rng_states,
 * ray_index_base) and what it wrote (d_rays).  The camera must not be updated between the two calls.  dsx = dsy = 1 returns the
 * raw Jacobian columns.  d_out: n records in device memory, 16-byte aligned.  Asynchronous on `stream`, with the threading
 * contract of zoic_create_rays_device.  ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for a NULL or
 * misaligned pointer; n = 0 returns ZOIC_OK. */
zoic_status zoic_ray_differentials_device(zoic_camera *cam, uint64_t n, const float *d_samples, const uint32_t *d_rng_states,
                                          uint64_t ray_index_base, const zoic_ray *d_rays, float dsx, float dsy,
                                          zoic_ray_differential *d_out, void *stream);
/* zoic_create_rays_arnold with traced derivative fields: origin, dir and weight[3] of every row are bit-identical to that
 * call's; dOdx, dOdy, dDdx, dDdy are the differentials above, scaled by the row's own input dsx / dsy. */
zoic_status zoic_create_rays_arnold_differentials(zoic_camera *cam, uint64_t n, const zoic_camera_input *inputs,
                                                  zoic_camera_output *outputs, uint64_t ray_index_base);
/* ---- rays at a wavelength per ray: chromatic aberration (opt-in; csrc/spectral.hpp has the full definition) -----------------
 * Each medium behind interface i (trace order, rear first) gets a two-term Cauchy index through its d-line index n_d (the
 * prescription's ior) and its Abbe number V (the prescription's fifth column, zoic.cpp:524, or zoic_camera_set_abbe_numbers):
 *   n_i(lambda) = n_d,i + B_i (1/lambda^2 - 1/587.5618^2),  B_i = (n_d,i - 1) / (V_i (1/486.1327^2 - 1/656.2725^2))
 * (B_i = 0 for air, a 4-column prescription or V <= 0).  Every interface applies the reference's eta and TIR rules (zoic.cpp:1013,
 * 1019) to the ray's own indices.  The exit-pupil LUT, the focus, the focal-length rescale and the bokeh tables stay those of the
 * d-line: the camera is focused at 587.5618 nm and other colours show longitudinal chromatic aberration. */
/* zoic_create_rays_device with a wavelength per ray: d_wavelengths = n f32 in nanometres in device memory, 4-byte aligned; every other
 * argument, the stream semantics, the retry streams keyed by ray index, the counters and the threading contract are that call's.
 * RAYTRACED: the model above (STRICT: the reference's arithmetic on the per-ray indices; at lambda = 587.5618 the records are
 * zoic_create_rays_device's bit for bit; FAST modes: decision-safe as there).  THINLENS and NONE ignore the wavelength: their records
 * (or NONE's error) are zoic_create_rays_device's.  A wavelength outside [360, 830] or NaN rejects that ray only: origin = dir = +0.0,
 * weight 0, flags == 0x80 (bit 7), and no counter counts it.  The differentials of these records come from
 * zoic_ray_differentials_spectral_device (zoic_ray_differentials_device replays the d-line trace).  ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for a NULL or misaligned pointer;
 * n = 0 returns ZOIC_OK. */
zoic_status zoic_create_rays_spectral_device(zoic_camera *cam, uint64_t n, const float *d_samples, const float *d_wavelengths,
                                             const uint32_t *d_rng_states, uint64_t ray_index_base, zoic_ray *d_rays, void *stream);
/* ---- hero-wavelength rays: k wavelengths through ONE lens point per sample (opt-in; csrc/hero.hpp has the full definition) ------
 * A spectral renderer carries a hero wavelength and a few companions per camera sample.  k spectral calls on the same samples run k
 * retry loops, and where a try passes at one wavelength and is clipped or totally reflected at another the colours of one sample
 * leave through different lens points.  This call runs the retry loop once, at the hero's wavelength, and sends the companions
 * through the hero's lens point.
 *   d_wavelengths : n x k f32 (nm) in device memory, 4-byte aligned, sample-major, the hero first: d_wavelengths[i*k + j]
 *   d_rays        : n x k zoic_ray records in device memory, 16-byte aligned, sample-major: record (i, j) at d_rays[i*k + j]
 *   every other argument as zoic_create_rays_spectral_device's; 1 <= k <= ZOIC_HERO_MAX_WAVELENGTHS.
 * Column 0 (the hero) is the record zoic_create_rays_spectral_device writes for sample i at d_wavelengths[i*k], bit for bit: ray i
 * draws its retries from the stream keyed by ray_index_base + i (i, not i*k) or from d_rng_states[i], and the camera's counters move
 * exactly as that call moves them.  With k = 1 the call IS that call.
 * Columns j >= 1 (the companions) of a hero with weight != 0: the hero's accepted try fixes the start -- the sensor point and the lens
 * point after the exit-pupil transform, the (o, d) the hero's trace began with -- and that start is traced ONCE through every
 * interface at d_wavelengths[i*k + j], with the trace the hero's tries use in the camera's precision mode (STRICT: the reference's
 * arithmetic on the per-ray indices; FAST modes: decision-safe, a trace that meets a clip inside a guard band is taken again in
 * STRICT arithmetic from the same start; a fastRunsStrict camera runs STRICT).  A companion that comes through gets origin and dir after
 * the final flip, the hero's weight and the hero's flags (tries, retried bit, LUT bit; bit 8 clear).  One that misses an interface, is
 * clipped at a housing or the stop, or is totally reflected gets origin = dir = +0.0, weight 0 and flags = the hero's flags |
 * ZOIC_RAY_COMPANION_LOST; no retry is drawn for it.  A companion at the hero's own wavelength is the hero's record bit for bit.
 * Companions of a hero with weight 0 (out of tries, a dead pixel) get +0.0 everywhere and flags = the hero's flags | bit 8.  So do
 * those of a hero whose weight comes from the reference's NaN ray (a draw on the disk's centre on a ray no retry can save, 2e-15 per
 * draw: its record is NaN and there is no start to share).
 * Companions touch no counter (their total reflections are not counted) and advance no retry stream.
 * A companion wavelength outside [360, 830] or NaN rejects that column only (all zero, flags == 0x80); an invalid hero wavelength
 * rejects the whole row (all k records zero with flags == 0x80) and nothing is counted for it.
 * THINLENS ignores the wavelengths: every valid column holds the record zoic_create_rays_device writes for sample i (bit 8 clear),
 * invalid columns and rows are rejected as above, and the counters are those of one spectral call on column 0.  NONE: that call's error.
 * Asynchronous on `stream`, with the threading contract of zoic_create_rays_device.  One exception, THINLENS with k > 1 only: the
 * thin-lens records are staged in ONE buffer per camera (n x 32 bytes, kept until zoic_camera_destroy), so such calls of one camera
 * run one after the other on the device whatever their streams, and a call with a larger n than any before waits on the host for the
 * previous one before it grows the buffer.  Results do not depend on it.  RAYTRACED calls use no scratch and never wait for each other.  ZOIC_ERR_INVALID_ARGUMENT for k = 0 or
 * k > ZOIC_HERO_MAX_WAVELENGTHS (checked first, on every camera) and for a NULL or misaligned pointer (d_rng_states may be NULL);
 * ZOIC_ERR_NO_DEVICE on a tables-only camera; ZOIC_ERR_NOT_UPDATED before an update; n = 0 returns ZOIC_OK.
 * Not covered: the tiles, the Arnold-layout calls, zoic_create_rays_host, zoic_frame_*.
 * Downstream, the rows form: the passes over records that already exist take the n x k records of this call as R = n*k rows of
 * a k = 1 call.  Row r = i*k + j has sample d_samples[i] and stream d_rng_states[i] (both repeated k times), wavelength
 * d_wavelengths[i*k + j] and record d_rays[i*k + j] (both arrays as they are).  In this form zoic_ray_differentials_spectral_device
 * gives every companion its own screen tangents and wavelength tangent, zoic_ray_transmittance_device (k = 1) the bits of its k >= 2
 * form, zoic_create_ghost_rays_device the ghosts of each colour, and zoic_trace_back_rays_spectral_device and
 * zoic_trace_back_jacobian_spectral_device take the records as they are (they read no sample and no stream).  A companion record carries
 * the hero's weight and flag word, so its replay is the hero's accepted try; a lost or rejected record has weight 0 and gets the
 * pass's dead result (+0.0; ZOIC_GHOST_NO_START).  The rows need the streams PER ROW: ray_index_base cannot name them, row r would
 * draw from the stream keyed by ray_index_base + r, the hero's is keyed by ray_index_base + i.  Where this call was given
 * d_rng_states == NULL, build the states the library derives -- rng_for_ray(seed, ray_index_base + i) of csrc/optics.hpp, in Python
 * zoic_amd.workloads.ray_rng_states(n, seed, ray_index_base); seed 1 unless zoic_camera_set_seed was called -- and repeat each k
 * times.  Without per-row states: the n-row call on column 0's records with column j's wavelengths and the original
 * d_rng_states / ray_index_base gives column j's differentials and ghosts wherever companion (i, j) came through (mask by its weight).
 * THINLENS: the tangents of every valid column are column 0's, the wavelength tangent is +0.0. */
#define ZOIC_HERO_MAX_WAVELENGTHS 8
#define ZOIC_RAY_COMPANION_LOST 0x100u   /* zoic_ray flags bit 8 */
zoic_status zoic_create_rays_hero_device(zoic_camera *cam, uint64_t n, uint32_t k, const float *d_samples,
                                         const float *d_wavelengths, const uint32_t *d_rng_states, uint64_t ray_index_base,
                                         zoic_ray *d_rays, void *stream);
/* ---- traced ray differentials of spectral records (opt-in; csrc/differentials_spectral.hpp has the full definition) ----------
 * The differentials above for the path a spectral record took: the accepted try is replayed and traced with every interface's
 * eta = n_i(lambda) / n_i+1(lambda) at the ray's own wavelength (one correctly rounded division, in every precision mode: STRICT and
 * FAST cameras give bitwise-equal results on rays whose tries agree).  At lambda = 587.5618, and on a lens without V-numbers at any
 * valid wavelength, d_out is zoic_ray_differentials_device's bit for bit.
 * d_chromatic (optional) receives the derivative of the same path with respect to the wavelength, PER NANOMETRE, with the sensor
 * point and the lens point L held fixed: dO/dlambda and dD/dlambda, after the final flip like the other tangents.  Its only source is
 * the indices' slope, dn_i/dlambda = -2 B_i / lambda^3; dsx / dsy never scale it.  It is traced in f64 (an achromat's crown and flint
 * contributions cancel in it) and returned as f32.  A hero-wavelength renderer shifts its companion
 * wavelengths' rays with it, a footprint estimate widens by it for colour fringes.
 * THINLENS ignores the wavelength (d_out as zoic_ray_differentials_device, +0.0 in d_chromatic); NONE gives zeros.  A record of
 * weight 0 (among them the rejected ones, flags 0x80) gets +0.0 everywhere, and so does every row whose wavelength HERE is outside
 * [360, 830] or NaN, whatever its record says.  The dispersion table is read at the call: a zoic_camera_set_abbe_numbers override
 * holds from the next call on (use the one the records were made with). */
/* zoic_ray_differentials_device for the records of zoic_create_rays_spectral_device: pass what that call was given
 * (d_samples, d_wavelengths, d_rng_states, ray_index_base) and what it wrote (d_rays).
 * d_chromatic: NULL, or n x 2 zoic_vec3 (dO/dlambda, dD/dlambda per nm; device memory, 8-byte aligned).
 * Stream semantics, threading contract and the other pointers' alignment as zoic_ray_differentials_device; d_wavelengths 4-byte
 * aligned.  ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for a NULL or misaligned pointer (d_wavelengths may not
 * be NULL); n = 0 returns ZOIC_OK. */
zoic_status zoic_ray_differentials_spectral_device(zoic_camera *cam, uint64_t n, const float *d_samples,
        const float *d_wavelengths, const uint32_t *d_rng_states, uint64_t ray_index_base, const zoic_ray *d_rays,
        float dsx, float dsy, zoic_ray_differential *d_out, zoic_vec3 *d_chromatic, void *stream);
/* The dispersion table of the camera's lens (works on a ZOIC_DEVICE_NONE camera): returns the surface count and writes up to
 * `capacity` entries, trace order (rear first), of n_d (after the 0 -> 1.0 fix, zoic.cpp:937-940), V (the override if one is set)
 * and B (nm^2) into the arrays that are not NULL; -1 for a NULL camera or a negative capacity. */
int zoic_camera_get_dispersion(const zoic_camera *cam, int capacity, float *ior_d, float *abbe, float *cauchy_b);
/* V-numbers for the dispersion table, in FILE order (front to rear, as a prescription lists them): gives glass data to 4-column
 * prescriptions.  count = 0 clears the override (V may be NULL).  A count that differs from the loaded lens's surface count returns
 * ZOIC_ERR_INVALID_ARGUMENT, here and at every zoic_camera_update while the override is set.  Changes nothing but the dispersion table. */
zoic_status zoic_camera_set_abbe_numbers(zoic_camera *cam, int count, const float *V);
/* ---- Fresnel transmittance of traced rays (opt-in; csrc/transmittance.hpp has the full definition) --------------------------------
 * The share of unpolarised light the lens's interfaces let through along the path a record took: T = the product over the interfaces
 * of 1 - (R_s + R_p) / 2, with every interface's indices at the ray's own wavelength (the dispersion table above), bare or with a
 * single-layer film (zoic_camera_set_coatings).  No absorption.  The accepted try is replayed once per sample and traced in the STRICT
 * arithmetic in every precision mode.  A pass over records that already exist: it changes no record and no counter; multiply a
 * record's weight by its T.
 * Pass what the forward call was given (d_samples, d_wavelengths, d_rng_states, ray_index_base) and what it wrote (d_rays):
 *   k == 1, d_wavelengths == NULL   the records of zoic_create_rays_device, at the d-line (587.5618 nm);
 *   k == 1, d_wavelengths           the records of zoic_create_rays_spectral_device;
 *   k >= 2                          the records of zoic_create_rays_hero_device (d_wavelengths may not be NULL).
 * d_rays and d_transmittance are n x k, sample-major; 1 <= k <= ZOIC_HERO_MAX_WAVELENGTHS.  The start comes from the sample, column 0's
 * try count and the ray's retry stream; every column whose record has weight != 0 and whose wavelength is valid is traced from it at
 * its own wavelength.  Every other column gets +0.0: weight 0 (a lost companion, a rejected record) or a wavelength HERE outside
 * [360, 830] or NaN, whatever its record says.  A replayed path that does not come through (possible only for records of
 * ZOIC_PRECISION_FAST_UNCHECKED or for inputs that do not match the records) gets +0.0 too.
 * THINLENS: 1.0 where the record has weight != 0 and the wavelength is valid, else +0.0.  NONE: zeros.
 * The dispersion and film tables are read at the call.  Stream semantics, threading contract and alignment (d_transmittance 4-byte
 * aligned) as zoic_ray_differentials_spectral_device.  ZOIC_ERR_INVALID_ARGUMENT for k == 0 or k > ZOIC_HERO_MAX_WAVELENGTHS (checked
 * first) and for a NULL or misaligned pointer (d_rng_states may be NULL); ZOIC_ERR_NOT_UPDATED before an update; n = 0 returns ZOIC_OK. */
zoic_status zoic_ray_transmittance_device(zoic_camera *cam, uint64_t n, uint32_t k, const float *d_samples,
        const float *d_wavelengths, const uint32_t *d_rng_states, uint64_t ray_index_base, const zoic_ray *d_rays,
        float *d_transmittance, void *stream);
/* Single-layer coatings, one per interface in FILE order (front to rear): the film's index (it does not disperse) and the wavelength
 * lambda0 (nm) at which it is a quarter wave thick.  Index 0: uncoated (the default for every interface); any other entry needs a
 * finite index >= 1 and a finite lambda0 > 0, else ZOIC_ERR_INVALID_ARGUMENT.  An interface between equal media (the stop) ignores its
 * entry.  count = the surface count; 0 clears (the arrays may be NULL).  A count that differs from the loaded lens's surface count
 * returns ZOIC_ERR_INVALID_ARGUMENT, here and at every zoic_camera_update while the override is set.  Changes nothing but the film table. */
zoic_status zoic_camera_set_coatings(zoic_camera *cam, int count, const float *film_index, const float *film_lambda0_nm);
/* The film table of the camera's lens (works on a ZOIC_DEVICE_NONE camera): returns the surface count and writes up to `capacity`
 * entries, trace order (rear first), into the arrays that are not NULL; -1 for a NULL camera or a negative capacity. */
int zoic_camera_get_coatings(const zoic_camera *cam, int capacity, float *film_index, float *film_lambda0_nm);
/* Multilayer coatings (csrc/coating_stack.hpp has the full definition): per interface an optional stack of 1 to ZOIC_COATING_MAX_LAYERS
 * homogeneous, loss-free layers that do not disperse, each with an index and a physical thickness (nm).  The stack is evaluated by the
 * characteristic-matrix method at the ray's own angle and wavelength for both polarisations, and is honoured wherever the single film
 * is: zoic_ray_transmittance_device, the weights of zoic_create_ghost_rays_device, and the trace-back and splat transmittance calls,
 * host and device with the same bits.
 *   Order      interfaces in FILE order (front to rear) like zoic_camera_set_coatings; the arrays are count x ZOIC_COATING_MAX_LAYERS,
 *              row-major, and within an interface layer 0 adjoins the front-side medium.
 *   layers[i]  0 ... ZOIC_COATING_MAX_LAYERS.  0: no stack there, the interface's zoic_camera_set_coatings entry stays in force (or it
 *              is bare); otherwise the stack overrides that entry.  Every used index must be finite and in [1, 4], every used thickness
 *              finite and in (0, 1000] nm, else ZOIC_ERR_INVALID_ARGUMENT; entries past layers[i] are not looked at.
 *   count      the surface count; 0 clears (the arrays may be NULL).  A count that differs from the loaded lens's surface count returns
 *              ZOIC_ERR_INVALID_ARGUMENT, here and at every zoic_camera_update while the override is set.  A refused call changes nothing.
 *   Special    an interface between equal media (the stop) ignores its stack; where a layer carries no wave at the ray's angle
 *              ((n1 / n_layer)^2 sin^2 i >= 1) the interface is priced bare.
 * Read at the call: no update is needed.  Like zoic_camera_update it is a setter of the camera -- call it while no call on the camera
 * is in flight; on a device camera it uploads the table with a blocking copy that has landed when it returns.  Cameras without a
 * stack run the kernels they ran before and return the same bits. */
#define ZOIC_COATING_MAX_LAYERS 8
zoic_status zoic_camera_set_coating_stacks(zoic_camera *cam, int count, const int32_t *layers, const float *layer_index,
        const float *layer_thickness_nm);
/* The stack table of the camera's lens (works on a ZOIC_DEVICE_NONE camera): returns the surface count and writes up to `capacity`
 * interfaces, trace order (rear first), each interface's layers in the order a forward ray (rear to front) meets them, into the arrays
 * that are not NULL (layer_index and layer_thickness_nm: ZOIC_COATING_MAX_LAYERS per interface); -1 for a NULL camera or a negative
 * capacity. */
int zoic_camera_get_coating_stacks(const zoic_camera *cam, int capacity, int32_t *layers, float *layer_index, float *layer_thickness_nm);
/* ---- ghost rays (opt-in; csrc/ghost.hpp has the full definition) -------------------------------------------------------------------
 * The light the transmittance above subtracts, followed: reflected at one interface and again at another it reaches the sensor as a
 * ghost (flare discs, veiling glare).  One ghost belongs to one main record, one wavelength and one ordered pair of interfaces (a, b),
 * trace-order indices (rear first), a > b: scene light that reflects first at b, then at a.  It is traced from the record's accepted try
 * in three legs -- +z through interfaces 0 ... a-1 to a reflection at a, -z through a-1 ... b+1 to a reflection at b, +z through
 * b+1 ... count-1 and out of the front element -- with the sphere, the housing / stop clip, the per-wavelength indices and the films
 * of every interface visit, in one f32 arithmetic in every precision mode.
 * d_ghosts receives n x p zoic_ray records, sample-major (record i * p + j: sample i, pair j).  A traced ghost: origin on the front
 * interface and dir (unit length, dir.z < 0) out into the scene in the frame of the forward records, flags == ZOIC_GHOST_TRACED, and
 * weight in (0, 1] = its Fresnel throughput only: the product of the transmittances of every refraction, each at its own angle (the
 * interfaces between b and a are crossed three times), times R_a R_b, R = 1 - T of that interface from the incidence side, 1 where the
 * reflection is total.  Multiply the main record's weight (and whatever else the renderer gives that record) in.
 * A ghost that ends early: origin, dir and weight +0.0, bit 0 clear, ZOIC_GHOST_REASON(flags) one of the codes below,
 * ZOIC_GHOST_INTERFACE(flags) the trace-order index and ZOIC_GHOST_LEG(flags) the leg (0, 1, 2) where it ended.  The reasons decided
 * before the trace are tested in this order and carry interface 0, leg 0: MODEL, INVALID_PAIR, NO_START, WAVELENGTH; then NO_REFLECTION
 * (interface a on leg 0, else b on leg 1), then NON_FINITE, then the trace's own.
 * Pass what the forward call was given (d_samples, d_wavelengths, d_rng_states, ray_index_base) and what it wrote (d_rays, n records,
 * k == 1): d_wavelengths == NULL for the records of zoic_create_rays_device (the d-line, 587.5618 nm), else those of
 * zoic_create_rays_spectral_device.  pairs: p entries in HOST memory, 1 <= p <= ZOIC_GHOST_MAX_PAIRS, each a | b << 8; they are copied
 * into the launch, so the array may be reused at once.  A pair with a <= b or an index past the lens is no error of the call: its column
 * gets INVALID_PAIR.  More pairs are served by successive calls.
 * It changes no record, no counter and no existing call.  The dispersion and film tables are read at the call.  Stream semantics,
 * threading contract and pointer alignment as zoic_ray_transmittance_device (pairs 4-byte, d_ghosts 16-byte aligned).
 * ZOIC_ERR_INVALID_ARGUMENT for p == 0 or p > ZOIC_GHOST_MAX_PAIRS (checked first, on every camera) and for a NULL or misaligned
 * pointer (d_wavelengths and d_rng_states may be NULL); ZOIC_ERR_NO_DEVICE on a tables-only camera; ZOIC_ERR_NOT_UPDATED before an
 * update; n = 0 returns ZOIC_OK. */
#define ZOIC_GHOST_MAX_PAIRS 32
#define ZOIC_GHOST_TRACED 0x1u
#define ZOIC_GHOST_REASON(flags) (((flags) >> 8) & 0xFu)
#define ZOIC_GHOST_INTERFACE(flags) (((flags) >> 16) & 0x3Fu)
#define ZOIC_GHOST_LEG(flags) (((flags) >> 24) & 0x3u)
#define ZOIC_GHOST_PAIR(a, b) ((uint32_t)(a) | ((uint32_t)(b) << 8))
#define ZOIC_GHOST_MISS 1u           /* the path misses an interface's sphere */
#define ZOIC_GHOST_CLIPPED 2u        /* outside a housing or the stop */
#define ZOIC_GHOST_TIR 3u            /* totally reflected where it had to refract */
#define ZOIC_GHOST_TURNED 4u         /* the ray no longer travels in its leg's direction */
#define ZOIC_GHOST_NO_REFLECTION 5u  /* the two media of a or of b are equal at this wavelength (always so at the stop) */
#define ZOIC_GHOST_NON_FINITE 6u     /* a NaN / inf start or result */
#define ZOIC_GHOST_WAVELENGTH 7u     /* the wavelength is outside [360, 830] or NaN */
#define ZOIC_GHOST_NO_START 8u       /* the main record has weight 0 */
#define ZOIC_GHOST_MODEL 9u          /* THINLENS / NONE: a lens without interfaces has no ghosts */
#define ZOIC_GHOST_INVALID_PAIR 10u  /* a <= b, or an index past the lens */
zoic_status zoic_create_ghost_rays_device(zoic_camera *cam, uint64_t n, uint32_t p, const uint32_t *pairs, const float *d_samples,
        const float *d_wavelengths, const uint32_t *d_rng_states, uint64_t ray_index_base, const zoic_ray *d_rays,
        zoic_ray *d_ghosts, void *stream);
/* The pairs that can make a ghost (works on a ZOIC_DEVICE_NONE camera): returns the number of pairs a > b whose two interfaces each
 * separate unequal media at the d-line (0 for THINLENS / NONE and before an update) and writes up to `capacity` of them, packed
 * a | b << 8, ordered by a, then b; -1 for a NULL camera or a negative capacity.  pairs may be NULL with capacity 0. */
int zoic_camera_get_ghost_pairs(const zoic_camera *cam, int capacity, uint32_t *pairs);
/* camera_create_ray(node, input, output, tid), zoic.cpp:1752: the per-sample signature.  No launch per call: the sample goes
 * to a resident kernel through mapped pinned memory (csrc/mailbox.hip; ~7 us per call; the kernel retires by itself after 1 ms
 * without a call and is started again by the next one).  Re-entrant: every tid owns a retry stream that carries over from call
 * to call, so two samples that retry never see the same draws; tid 0's stream is the reference's process-global xor128 state
 * (seeded 123456789..., advanced by node_update's LUT build and by every retry), so ONE render thread reproduces the
 * reference's sequential output exactly (STRICT precision).
 * Output fields: as the reference, the call UPDATES the caller's AtCameraOutput in place -- origin, dir written; weight set to 0
 * (zoic.cpp:1825/1952) or multiplied by the exposure factor (zoic.cpp:1981-1987); dOdy/dDdy written for retried rays only;
 * dOdx/dDdx never touched -- whereas zoic_create_rays_arnold writes whole rows from a zero-initialised output with weight 1.
 * For an output that Arnold hands in (zeroed, weight 1) the two agree.  THINLENS is evaluated in the reference's arithmetic in
 * every precision mode here; under ZOIC_PRECISION_FAST with opticalVignettingDistance > 0 the batch entry points use the fast
 * arithmetic, so the same sample can differ in low-order bits between the two (decisions never differ). */
zoic_status zoic_camera_create_ray(zoic_camera *cam, const zoic_camera_input *input, zoic_camera_output *output,
                                   uint16_t tid);
/* ---- tiles: what a render thread buffers of camera_create_ray (zoic.cpp:1752), answered without a launch --------------------
 * A renderer works in buckets (Arnold: 64 x 64 pixels x AA^2 samples = 36 K ... 150 K samples per bucket and thread).  Served by
 * kernel launches such a batch costs 50-80 us of launch, stream and copy overhead whatever it carries; a zoic_tile goes to the
 * camera's RESIDENT kernel instead (csrc/mailbox.hip): the request is one 64-byte line in mapped page-locked memory, the kernel's
 * worker waves take 64 samples each at full lane width -- the same device functions, hence the same bits, as the batch kernels --
 * read the AtCameraInput rows and write the AtCameraOutput rows in place across PCIe, and the render thread spins on one word.
 *   zoic_tile_create  page-locked input / output arrays of `capacity` rows (<= ZOIC_TILE_MAX_SAMPLES) for render thread `tid`
 *                     (tile requests of tids 64 apart share a mailbox slot and are served one after the other);
 *   zoic_tile_inputs / _outputs   the arrays: the caller fills inputs[0 .. n) (the fields zoic reads: sx, sy, lensx, lensy);
 *   zoic_tile_submit  posts rows [0, n) and returns at once; ray i draws its retries from the stream keyed by
 *                     ray_index_base + i, exactly as zoic_create_rays_arnold does: outputs[i] equals that call's row bit for bit
 *                     (whole rows: origin, dir, weight[3], dOdy / dDdy for retried rays, zeros elsewhere);
 *   zoic_tile_wait    returns when outputs[0 .. n) are complete; zoic_tile_done polls (1 = complete, nothing pending).
 * One submit per tile at a time (a second submit waits for the first).  A tile belongs to one render thread; different tiles may
 * be used from different threads at once.  zoic_camera_update: wait for the camera's tiles first.  zoic_camera_destroy settles the
 * tiles still alive and DETACHES them: their arrays go with the camera (zoic_tile_inputs / _outputs / _rays / _samples return NULL,
 * zoic_tile_capacity 0), every call on them but zoic_tile_destroy fails with ZOIC_ERR_INVALID_ARGUMENT.
 * zoic_tile_done may be polled without a zoic_tile_wait in between (it restarts a resident kernel that retired under the poll); a
 * HIP error it runs into is reported by the next zoic_tile_wait / _submit.
 * zoic_camera_create_rays_tile is the one-call form for arrays the caller owns: page-locked mapped arrays (zoic_host_alloc /
 * zoic_host_register) are used in place, anything else is staged through the slot's own page-locked buffers (two 16 Ki-row
 * pieces in flight).  Any n.  Counters: tile rays count like every other ray.
 *   zoic_tile_set_rows(tile, ZOIC_TILE_ROWS_RAYS)  the tile's answer is n zoic_ray RECORDS (32 bytes: origin, dir, weight, flags --
 *                     what zoic_create_rays_device writes, bit for bit) at zoic_tile_rays() instead of n AtCameraOutput rows (84 bytes,
 *                     51 of them zeros or copies): with many render threads a tile costs what its rows cost on PCIe, and a
 *                     renderer that reads origin / dir / weight (dOdy = origin, dDdy = dir when flags bit 0 is set, zoic.cpp:1974-1977)
 *                     needs nothing else.  ZOIC_TILE_ROWS_ARNOLD (the default) switches back.  Between a wait and the next submit only.
 *   zoic_tile_set_inputs(tile, ZOIC_TILE_INPUTS_SAMPLES)  the tile is filled with 16-byte (sx, sy, lensx, lensy) samples at zoic_tile_samples()
 *                     -- the four fields zoic reads (zoic.cpp:1853-1854, 1870), what zoic_create_rays_device takes -- instead of 28-byte
 *                     AtCameraInput rows.  ZOIC_TILE_INPUTS_ARNOLD (the default) switches back.  Between a wait and the next submit only. */
#define ZOIC_TILE_MAX_SAMPLES 65536u
#define ZOIC_TILE_ROWS_ARNOLD 0
#define ZOIC_TILE_ROWS_RAYS 1
#define ZOIC_TILE_INPUTS_ARNOLD 0
#define ZOIC_TILE_INPUTS_SAMPLES 1
typedef struct zoic_tile zoic_tile;
zoic_status zoic_tile_create(zoic_camera *cam, uint32_t capacity, uint16_t tid, zoic_tile **out);
void        zoic_tile_destroy(zoic_tile *tile);
zoic_camera_input  *zoic_tile_inputs(zoic_tile *tile);
zoic_camera_output *zoic_tile_outputs(zoic_tile *tile);
uint32_t    zoic_tile_capacity(const zoic_tile *tile);
zoic_status zoic_tile_submit(zoic_tile *tile, uint32_t n, uint64_t ray_index_base);
zoic_status zoic_tile_wait(zoic_tile *tile);
int         zoic_tile_done(zoic_tile *tile);
zoic_status zoic_tile_set_rows(zoic_tile *tile, int rows);
const zoic_ray *zoic_tile_rays(const zoic_tile *tile);
zoic_status zoic_tile_set_inputs(zoic_tile *tile, int inputs);
float *zoic_tile_samples(zoic_tile *tile);   /* capacity x 4 floats: the same memory as zoic_tile_inputs */
zoic_status zoic_camera_create_rays_tile(zoic_camera *cam, uint32_t n, const zoic_camera_input *inputs, zoic_camera_output *outputs,
                                         uint64_t ray_index_base, uint16_t tid);
/* The same resident kernel for a GPU consumer's mid-size batch: n <= ZOIC_RESIDENT_MAX_SAMPLES (sx, sy, lensx, lensy) samples in DEVICE memory
 * -> n zoic_ray records in DEVICE memory, what zoic_create_rays_device(cam, n, d_samples, NULL, ray_index_base, d_rays, stream) writes, bit
 * for bit, without a kernel launch: a launch-based call costs 52-76 us whatever it carries; this one 30 us for 4096
 * samples (launch + synchronise: 90) and 68 us for 65 536 (115).  NOT stream-ordered: d_samples must be complete when the call is made (synchronise the stream that produced them), the
 * call returns when d_rays is complete and visible to any kernel launched afterwards.  Pieces of 65536 samples are served one after the
 * other on the mailbox slot of `tid` (several threads, several slots: 1.9 Grays/s from four): beyond a few hundred thousand samples per call
 * zoic_create_rays_device's one launch is the faster call. */
#define ZOIC_RESIDENT_MAX_SAMPLES 1048576u
zoic_status zoic_create_rays_device_resident(zoic_camera *cam, uint32_t n, const float *d_samples, zoic_ray *d_rays, uint64_t ray_index_base,
                                             uint16_t tid);
/* camera_reverse_ray, zoic.cpp:1992-1995: the reference returns false and writes nothing; so does this (returns 0) by default.
 * Opted in with zoic_camera_set_reverse_projection(cam, 1): returns flags & 1 of zoic_project_point and writes Ps (also when it
 * returns 0: then (+0, +0)); fov is ignored and relative_time is not written.  A camera that has no successful update returns 0. */
int zoic_camera_reverse_ray(const zoic_camera *cam, const zoic_vec3 *Po, float fov, float *Ps /* [2] */,
                            float *relative_time);
/* ---- reverse projection: scene points to screen samples (opt-in; csrc/reverse.hpp has the full definition) ------------------
 * Po is a point in the frame of the records the forward calls write (zoic_ray origin / dir after the reference's flips).  Ps = (sx, sy)
 * is the screen sample the forward calls would take:
 *   THINLENS   the sample whose lens-centre ray passes through Po: sx = Po.x / (-Po.z) / tan_fov, sy likewise; only for Po.z < 0.
 *   RAYTRACED  the sensor point (sx sw/2, sy sw/2, originShift), sw = sensorWidth, of the CHIEF ray through Po: the ray through the centre
 *              of the aperture stop, refracted at every interface (the near-vertex intersection of each sphere; the stop as the plane
 *              through its vertex; of several roots the one continuous with the paraxial solution).  A point on the axis gives (+0, +0).
 *              A camera outside the geometric domain of the FAST modes (negative focal-length rescale, or sensor in front of the rear
 *              vertex: see zoic_precision) projects no point; lensModel NONE neither.
 * Flags: bit 0 projected (Ps written); bit 1 the chief ray is clipped by some element's housing (Ps is still the chief ray's); bit 2
 * the sensor radius lies beyond the exit-pupil LUT's last key (forward rays there carry zoic_ray flag bit 6); bits 8-11 when bit 0 is
 * clear: the reason below.  A point that is not projected gets Ps = (+0, +0).
 * The arithmetic is f32 with correctly rounded square roots and reciprocals, the same on the host and on the device in every
 * precision mode: zoic_project_points_device and zoic_project_point give the same bits for the same point. */
#define ZOIC_PROJECTED 0x1u
#define ZOIC_PROJECT_CLIPPED 0x2u
#define ZOIC_PROJECT_PAST_LUT 0x4u
#define ZOIC_PROJECT_REASON(flags) (((flags) >> 8) & 0xFu)
enum {
    ZOIC_PROJECT_BEHIND = 1,         /* behind the lens (RAYTRACED: not in front of the front element's cap), or Po.z >= 0 (THINLENS) */
    ZOIC_PROJECT_NO_ROOT = 2,        /* no chief ray: a sphere missed or total internal reflection on every candidate (or Ps overflows) */
    ZOIC_PROJECT_NON_FINITE = 3,     /* a NaN or infinite coordinate */
    ZOIC_PROJECT_MODEL_NONE = 4,     /* lensModel NONE */
    ZOIC_PROJECT_OUTSIDE_DOMAIN = 5, /* RAYTRACED camera outside the geometric domain above */
    ZOIC_PROJECT_WAVELENGTH = 6      /* the spectral calls below: the point's wavelength is outside [360, 830] nm or NaN */
};
/* n points (packed float3, device memory, 4-byte aligned) -> n (sx, sy) pairs (device memory, 8-byte aligned) and, unless d_flags is
 * NULL, n flag words (device memory).  Works whatever zoic_camera_set_reverse_projection says.  Asynchronous on `stream`.
 * ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for a NULL, misaligned or non-device pointer; n = 0 returns ZOIC_OK. */
zoic_status zoic_project_points_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */, float *d_screen /* n x 2 */,
                                       uint32_t *d_flags /* may be NULL */, void *stream);
/* The host build of the same code for one point (no GPU round trip; works on a ZOIC_DEVICE_NONE camera).  flags may be NULL. */
zoic_status zoic_project_point(const zoic_camera *cam, const zoic_vec3 *Po, float *Ps /* [2] */, uint32_t *flags);
/* Off by default.  On: zoic_camera_reverse_ray answers with zoic_project_point (see there).  A _set_* call. */
zoic_status zoic_camera_set_reverse_projection(zoic_camera *cam, int enable);

/* ---- trace-back: camera rays to their screen samples (opt-in; csrc/traceback.hpp has the full definition) --------------------
 * The reverse projection above answers for the CHIEF ray of a point.  These two calls answer for ONE PARTICULAR ray arriving at the
 * front element: does it get through the housings and the stop, and on which screen sample does it land?  (What a light tracer, a
 * splatter or a bidirectional integrator needs for depth of field; how lens points are drawn and weighted is the caller's.)
 * Input: a camera ray as the forward calls write it -- zoic_ray origin and dir in the frame of the records, dir pointing away from the
 * camera into the scene (dir.z < 0), any length; origin any point of the ray's line in front of the lens (a forward record's origin
 * lies on the front surface; a light tracer passes its scene point and dir = point - lens point).  weight and flags are not read.
 *   RAYTRACED  the ray is followed back through every interface, front to rear: the intersection the forward trace takes, the forward
 *              kernels' housing / stop limits (the stop's holds min(housing, userApertureRadius)), Snell with the true ratio of the
 *              media; the stop is the reference's sphere of |R| ~ 1e4 cm.  Ps = the point where it meets the sensor plane z = originShift,
 *              divided by sensorWidth / 2 in x AND y (zoic.cpp:1853-1854).  Nothing is clipped at the sensor: the caller knows its frame
 *              (|sx| <= 1, |sy| <= 1 / aspect).  Cameras outside the geometric domain of the FAST modes (see zoic_precision) trace no ray.
 *   THINLENS   with useDof: the lens point P = the line's crossing of z = 0 must lie within apertureRadius (the forward path's disk
 *              sampler overshoots that disk by up to 0.1 % on 0.06 % of its rays: those records are refused) and, with
 *              opticalVignettingDistance > 0, pass the test of
 *              zoic.cpp:1297-1305; Ps = the line's crossing of z = -focalDistance divided by focalDistance tan_fov.  Without DOF (a pinhole passes no generic ray) and for lensModel NONE: ZOIC_TRACE_BACK_MODEL
 *              (zoic_project_point answers there).
 * Flags: bit 0 traced back (the ray reaches the sensor unclipped; Ps written); bit 2 the sensor radius lies beyond the exit-pupil LUT's
 * last key (as ZOIC_PROJECT_PAST_LUT); bits 8-11 when bit 0 is clear: the reason below; bits 16-21, for MISS / CLIPPED / TIR: the index
 * (trace order, rear first: the order of zoic_lens_info) of the interface where the ray ended.  A ray that is not traced back gets
 * Ps = (+0, +0).
 * The arithmetic is f32 with correctly rounded square roots and reciprocals, the same on the host and on the device in every
 * precision mode: zoic_trace_back_rays_device and zoic_trace_back_ray give the same bits for the same ray. */
#define ZOIC_TRACED_BACK 0x1u
#define ZOIC_TRACE_BACK_PAST_LUT 0x4u
#define ZOIC_TRACE_BACK_REASON(flags) (((flags) >> 8) & 0xFu)
#define ZOIC_TRACE_BACK_INTERFACE(flags) (((flags) >> 16) & 0x3Fu)
enum {
    ZOIC_TRACE_BACK_AWAY = 1,           /* dir.z >= 0, or the start point is not in front of the front element's cap (THINLENS: origin.z > 0) */
    ZOIC_TRACE_BACK_MISS = 2,           /* the ray misses an interface's sphere */
    ZOIC_TRACE_BACK_CLIPPED = 3,        /* outside an interface's housing, the stop or the thin lens's aperture / vignetting test */
    ZOIC_TRACE_BACK_TIR = 4,            /* total internal reflection */
    ZOIC_TRACE_BACK_NON_FINITE = 5,     /* a NaN or infinite coordinate, dir = 0, or Ps overflows */
    ZOIC_TRACE_BACK_MODEL = 6,          /* lensModel NONE, or THINLENS without useDof */
    ZOIC_TRACE_BACK_OUTSIDE_DOMAIN = 7, /* RAYTRACED camera outside the geometric domain */
    ZOIC_TRACE_BACK_WAVELENGTH = 8      /* the spectral calls below: the ray's wavelength is outside [360, 830] nm or NaN */
};
/* n zoic_ray records (device memory, 16-byte aligned) -> n (sx, sy) pairs (device memory, 8-byte aligned) and, unless d_flags is NULL,
 * n flag words (device memory).  d_rays may be the buffer zoic_create_rays_device wrote, on the same stream, without a copy.
 * Asynchronous on `stream`, with the threading contract of zoic_project_points_device; touches no counter and no retry stream.
 * ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for a NULL, misaligned or non-device pointer; ZOIC_ERR_NO_DEVICE on
 * a tables-only camera; n = 0 returns ZOIC_OK. */
zoic_status zoic_trace_back_rays_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays, float *d_screen /* n x 2 */,
                                        uint32_t *d_flags /* may be NULL */, void *stream);
/* The host build of the same code for one ray (no GPU round trip; works on a ZOIC_DEVICE_NONE camera).  flags may be NULL. */
zoic_status zoic_trace_back_ray(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir, float *Ps /* [2] */,
                                uint32_t *flags /* may be NULL */);

/* ---- the backward paths at a wavelength per item (opt-in; csrc/backward_spectral.hpp has the full definition) ----------------
 * zoic_create_rays_spectral_device traces every ray at a wavelength of its own; these four calls are zoic_trace_back_* and
 * zoic_project_point* for such rays and points, so that a light tracer, a splatter or a bidirectional integrator meets the camera the
 * forward pass rendered with: a spectral record traced back at its wavelength returns to its sample, and a point splatted in blue and in
 * red lands on the two pixels the forward pass puts it on (lateral colour).
 *   Index   the medium behind interface i has n_i(lambda) = n_d,i + B_i (1/lambda^2 - 1/lambda_d^2) in the forward kernels' own f32
 *           operations (csrc/spectral.hpp spectral_dl, spectral_ior), n_d and B as zoic_camera_get_dispersion reports them (a
 *           zoic_camera_set_abbe_numbers override is honoured, from the next call on); in front of the front element exactly 1.0f.
 *   Ratio   every interface takes the true ratio of its two media, as the d-line calls' tables do: trace-back n_front / n_rear,
 *           projection n_rear / n_front towards the front and n_front / n_rear towards the rear, each ONE correctly rounded f32 division.
 *           On the device that is the compiler's IEEE division (v_div_scale / v_rcp / FMA refinement / v_div_fmas / v_div_fixup: the
 *           library is built without fast-math), on the host divss: the same bits (csrc/backward_spectral.hpp, "Division").
 *   The d-line's own: geometry, housings, the stop limit, the sensor plane (originShift), the focal-length rescale, the LUT flag, the
 *           domain gate, the cap test, the projection's paraxial first guess, every step that reads no index.  The camera is focused at
 *           587.5618 nm, as on the forward side.
 *   At wavelength 587.5618f every index is n_d exactly: Ps and flags equal the d-line calls' bit for bit, for every input.
 *   A wavelength outside [360, 830] nm, or NaN, rejects that item alone, before anything else is looked at: Ps = (+0, +0), bit 0 clear,
 *           reason ZOIC_TRACE_BACK_WAVELENGTH / ZOIC_PROJECT_WAVELENGTH.  THINLENS and NONE cameras ignore the wavelength apart from
 *           that: their answers are the d-line calls'.
 * d_wavelengths: n f32 (nm), device memory, 4-byte aligned.  Every other argument, the error codes, the stream semantics and the
 * threading contract are those of the d-line call of the same name; no counter and no retry stream is touched; host and device give the
 * same bits for the same item in every precision mode.  zoic_camera_reverse_ray is unchanged (the d-line projection). */
zoic_status zoic_trace_back_rays_spectral_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays, const float *d_wavelengths /* n */,
                                                 float *d_screen /* n x 2 */, uint32_t *d_flags /* may be NULL */, void *stream);
zoic_status zoic_trace_back_ray_spectral(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir, float wavelength_nm,
                                         float *Ps /* [2] */, uint32_t *flags /* may be NULL */);
zoic_status zoic_project_points_spectral_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */,
                                                const float *d_wavelengths /* n */, float *d_screen /* n x 2 */,
                                                uint32_t *d_flags /* may be NULL */, void *stream);
zoic_status zoic_project_point_spectral(const zoic_camera *cam, const zoic_vec3 *Po, float wavelength_nm, float *Ps /* [2] */,
                                        uint32_t *flags /* may be NULL */);

/* ---- the trace-back Jacobian: dPs / d(origin, dir) (opt-in; csrc/traceback_jacobian.hpp has the full definition) ---------------
 * The trace-back calls above answer WHERE a ray lands.  These four answer how that place moves with the ray, which is what lets a
 * trace-back carry energy: a light tracer or a splatter divides by |det dPs/d(omega)| at a fixed origin, a bidirectional connection to
 * a point on the front element needs dPs/d(origin).  For a ray that is traced back (bit 0 of its flags)
 *       J = d(sx, sy) / d(origin.x, origin.y, origin.z, dir.x, dir.y, dir.z)
 * 2 x 6, row-major: the six derivatives of sx, then the six of sy.  dir is differentiated as given, at any length.
 *   Map        J is the derivative of the exact map of the trace-back: the move along the line to the front vertex plane, the
 *              normalisation, at every interface the hit, the normal and Snell, then the sensor plane; tangents after Igehy's transfer
 *              and refraction, carried along the one trace (four of them: the rays are a 4-dimensional manifold).
 *   Identities J_o . dir = 0 and J_d . dir = 0 (J_o, J_d: the first and the last three columns): moving the origin along the line
 *              changes nothing, scaling dir changes nothing.  The cap test, the LUT flag and the clip decisions have no derivative.
 *   THINLENS   (with useDof) the closed form: with tau = -(origin.z + focalDistance) / dir.z and I = 1 / (focalDistance tan_fov),
 *              d sx/d origin.x = I, d sx/d origin.z = -(dir.x / dir.z) I, d sx/d dir.x = tau I, d sx/d dir.z = -tau (dir.x / dir.z) I.
 *   Spectral   the wavelength is held fixed (no tangent); an invalid one gives ZOIC_TRACE_BACK_WAVELENGTH.  At 587.5618f the spectral
 *              calls give the d-line calls' bits.
 * Ps and flags are those of zoic_trace_back_ray / zoic_trace_back_ray_spectral bit for bit, for every input.  A ray that is not traced
 * back gets Ps = (+0, +0) and twelve +0.0.  J is not clipped: an entry of a ray of extreme scale may be infinite, and one that is not a
 * number is written as the quiet NaN 0x7fc00000.
 * The arithmetic is the trace-back's (f32, correctly rounded square roots, reciprocals and divisions), the same on the host and on the
 * device in every precision mode: the device calls and the host calls give the same bits for the same ray, J included.
 * d_jacobian: n x 12 floats, device memory, 16-byte aligned.  Every other argument, the error codes (ZOIC_ERR_NOT_UPDATED before an
 * update; ZOIC_ERR_INVALID_ARGUMENT for a NULL, misaligned or non-device pointer, before any launch; ZOIC_ERR_NO_DEVICE on a tables-only
 * camera; n = 0 returns ZOIC_OK), the stream semantics and the threading contract are those of zoic_trace_back_rays_device /
 * zoic_trace_back_rays_spectral_device; no counter and no retry stream is touched. */
zoic_status zoic_trace_back_jacobian_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays, float *d_screen /* n x 2 */,
                                            uint32_t *d_flags /* may be NULL */, float *d_jacobian /* n x 12 */, void *stream);
/* The host build of the same code for one ray (works on a ZOIC_DEVICE_NONE camera).  flags may be NULL. */
zoic_status zoic_trace_back_ray_jacobian(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir, float *Ps /* [2] */,
                                         uint32_t *flags /* may be NULL */, float *J /* [12] */);
zoic_status zoic_trace_back_jacobian_spectral_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays, const float *d_wavelengths /* n */,
                                                     float *d_screen /* n x 2 */, uint32_t *d_flags /* may be NULL */,
                                                     float *d_jacobian /* n x 12 */, void *stream);
zoic_status zoic_trace_back_ray_jacobian_spectral(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir, float wavelength_nm,
                                                  float *Ps /* [2] */, uint32_t *flags /* may be NULL */, float *J /* [12] */);

/* ---- pupil bounds: the lens area and the blur spot of a scene point (opt-in; csrc/pupil_bounds.hpp has the full definition) ------
 * The trace-back calls above leave the step before them to the caller: how lens points are drawn.  Drawn from the whole front element,
 * almost every ray of a stopped-down or vignetted camera is refused at the stop.  These four calls answer, for a scene point P (the
 * frame of the records, as zoic_project_point takes it): which part of the lens does P see, and how big is its blur spot on the sensor
 * -- the circle of confusion with its cat's eye, and the vignetting.  Deterministic: no random number, no weight.
 *   Aims     lattice x lattice points A, the cell centres of the square [-R, R]^2 across the axis: RAYTRACED on the front vertex plane
 *            with R the front element's housing radius, THINLENS with useDof on the lens plane z = 0 with R = apertureRadius.
 *            ax = (2 ix + 1 - lattice) R / lattice, ay likewise.  lattice is 8, 16 or 32.
 *   Ray      origin = P, dir = P - A, taken back by zoic_trace_back_ray, spectral: by zoic_trace_back_ray_spectral at the point's wavelength.
 *   Passing  an aim passes if its ray is traced back (ZOIC_TRACED_BACK) and, where a window (sx0, sy0, sx1, sy1) is given,
 *            sx0 <= sx <= sx1 and sy0 <= sy <= sy1.  A NaN window bound passes nothing.  window = NULL: no window.
 *   Record   aim: min ax, min ay, max ax, max ay over the passing aims, each side grown by one pitch 2 R / lattice and clamped to +-R.
 *            screen: min sx, min sy, max sx, max sy over the passing aims, not grown: the box of the blur spot.
 *            count: the passing aims; lattice: lattice^2, so that count / lattice x 4 R^2 is the pupil's area as seen from P.
 *            flags: bit 0 (ZOIC_PUPIL_SOME) at least one aim passes; bits 16-31 the OR over the refused aims of
 *            ZOIC_PUPIL_REFUSED(reason), reason a ZOIC_TRACE_BACK_* code, and 0 for an aim that traced back but landed outside the window.
 *            With no aim passing, aim and screen are all +0.
 *   Refused wholesale: lensModel NONE, THINLENS without useDof, a camera outside the geometric domain, a non-finite P, a P behind the front
 *            element's cap, an invalid wavelength.  Not an error: count = 0 and the bit of that reason.
 * The bounds are statements about the lattice, not a guarantee: every passing lattice aim lies in `aim`, but a sliver of pupil thinner
 * than a pitch can lie outside the grown box (DESIGN 4.17 has the measured share).  Draw lens points in `aim`, trace each ray back as before
 * (zoic_trace_back_jacobian_device gives the change of measure); how they are weighted stays the caller's.
 * Every output is a minimum, a maximum, a count or an OR over the trace-back's own bits: the device calls and the host calls give the same
 * record for the same point in every precision mode.
 * d_points: n x 3 floats, device memory, 4-byte aligned; d_wavelengths: n f32 (nm), device memory; window: 4 floats of HOST memory, read
 * during the call, or NULL; d_bounds: n records, device memory, 16-byte aligned.  Asynchronous on `stream`, with the threading contract of
 * zoic_trace_back_rays_device; no record, no counter and no retry stream is touched.  ZOIC_ERR_NOT_UPDATED before an update;
 * ZOIC_ERR_INVALID_ARGUMENT for a NULL, misaligned or non-device pointer or a lattice that is not 8, 16 or 32, before any launch;
 * ZOIC_ERR_NO_DEVICE on a tables-only camera; n = 0 returns ZOIC_OK. */
typedef struct zoic_pupil_bounds {
    float aim[4];    /* min ax, min ay, max ax, max ay (cm), grown by a pitch and clamped */
    float screen[4]; /* min sx, min sy, max sx, max sy */
    uint32_t count;
    uint32_t lattice;
    uint32_t flags;
    uint32_t reserved; /* 0 */
} zoic_pupil_bounds; /* 48 bytes */
#define ZOIC_PUPIL_SOME 0x1u
#define ZOIC_PUPIL_OUTSIDE_WINDOW 0 /* the reason of an aim that traced back but landed outside the window */
#define ZOIC_PUPIL_REFUSED(reason) (1u << (16 + (reason)))
zoic_status zoic_pupil_bounds_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */, int lattice,
                                     const float *window /* [4], host, may be NULL */, zoic_pupil_bounds *d_bounds /* n */, void *stream);
zoic_status zoic_pupil_bounds_spectral_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */,
                                              const float *d_wavelengths /* n */, int lattice, const float *window /* [4], host, may be NULL */,
                                              zoic_pupil_bounds *d_bounds /* n */, void *stream);
/* The host build of the same code for one point (works on a ZOIC_DEVICE_NONE camera). */
zoic_status zoic_pupil_bounds_point(const zoic_camera *cam, const zoic_vec3 *Po, int lattice, const float *window /* [4] or NULL */,
                                    zoic_pupil_bounds *bounds);
zoic_status zoic_pupil_bounds_point_spectral(const zoic_camera *cam, const zoic_vec3 *Po, float wavelength_nm, int lattice,
                                             const float *window /* [4] or NULL */, zoic_pupil_bounds *bounds);

/* ---- lens splats: a scene point through drawn aims in its pupil box to the screen (opt-in; csrc/splat.hpp has the full definition) --
 * The device call that puts the backward calls together for a point splatter or a light tracer: from each scene point P and its
 * pupil-bounds record B (as zoic_pupil_bounds_device wrote it, read in place), m rays towards m aims in B's `aim` box, each traced back
 * with its Jacobian, of which the four numbers a splatter keeps are written.  Deterministic: the caller brings the numbers u, nothing
 * is drawn, weighted or accumulated here.
 *   Empty box  B.count == 0 or ZOIC_PUPIL_SOME clear: nothing is traced; the record is all +0 but flags = ZOIC_SPLAT_NO_BOX (bit 12, a
 *              bit the trace-back's flag word leaves free).
 *   Aim        ax = aim[0] + u0 (aim[2] - aim[0]), then clamped to [aim[0], aim[2]] by two selects; ay likewise with aim[1], aim[3], u1:
 *              uniform in the box for u uniform in [0, 1)^2, on the box's edge for u outside.  A NaN u gives a NaN aim, which the trace
 *              refuses (ZOIC_TRACE_BACK_NON_FINITE).  The aims' plane is that of the pupil bounds.
 *   Ray        origin = P, dir = P - A, taken back by zoic_trace_back_ray_jacobian (spectral: zoic_trace_back_ray_jacobian_spectral at the
 *              point's wavelength): sx, sy and flags are that call's bits.
 *   Measures   for a traced ray (ZOIC_TRACED_BACK), +0 otherwise, with J that call's Jacobian:
 *              area  = J[3] J[10] - J[4] J[9] = det d(sx, sy) / d(ax, ay) at fixed P: screen area per cm^2 of the aims' plane.  With u
 *                      uniform, the density of the aims is 1 / |box| per cm^2.
 *              angle = area |dir|^3 / dir.z = dPs / d(omega), the value of solid_angle_measure(J, dir) (dir.z < 0: the sign is -area's).
 *              An entry that is not a number is the one quiet NaN 0x7fc00000.
 *   Record     ax, ay are written for every ray that was traced or refused by the trace, and are +0 with ZOIC_SPLAT_NO_BOX.
 *   m          m >= 1 aims per point, point-major: splat i = p m + j reads point p, bounds p, u[2 i], u[2 i + 1] and writes record i.
 * Every operation is a single correctly rounded f32 operation in a fixed order: the device calls and the host calls give the same
 * record for the same item in every precision mode.
 * d_points: n x 3 floats, device memory, 4-byte aligned; d_bounds: n records, device memory, 16-byte aligned; d_u: n x m x 2 floats,
 * device memory, 8-byte aligned; d_wavelengths: n f32 (nm), device memory; d_splats: n x m records, device memory, 16-byte aligned.
 * Asynchronous on `stream`, with the threading contract of zoic_pupil_bounds_device; no counter and no retry stream is touched.
 * ZOIC_ERR_NOT_UPDATED before an update; ZOIC_ERR_INVALID_ARGUMENT for m = 0 with n > 0, for n m >= 2^58 and for a NULL, misaligned or
 * non-device pointer, before any launch: d_splats is not written; ZOIC_ERR_NO_DEVICE on a tables-only camera; n = 0 returns ZOIC_OK. */
typedef struct zoic_splat {
    float sx, sy;      /* the screen sample */
    float ax, ay;      /* the aim (cm) on the pupil bounds' plane */
    float area;        /* det d(sx, sy) / d(ax, ay) */
    float angle;       /* dPs / d(omega) */
    uint32_t flags;    /* the trace-back's flag word, or ZOIC_SPLAT_NO_BOX */
    uint32_t reserved; /* 0 */
} zoic_splat; /* 32 bytes */
#define ZOIC_SPLAT_NO_BOX 0x1000u
zoic_status zoic_splat_points_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */, const zoic_pupil_bounds *d_bounds /* n */,
                                     uint32_t m, const float *d_u /* n x m x 2 */, zoic_splat *d_splats /* n x m */, void *stream);
zoic_status zoic_splat_points_spectral_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */,
                                              const zoic_pupil_bounds *d_bounds /* n */, const float *d_wavelengths /* n */, uint32_t m,
                                              const float *d_u /* n x m x 2 */, zoic_splat *d_splats /* n x m */, void *stream);
/* The host build of the same code for one point and its m aims (works on a ZOIC_DEVICE_NONE camera).  u and splats: host
 * memory, 4-byte aligned.  m = 0, a NULL pointer and a misaligned u or splats are ZOIC_ERR_INVALID_ARGUMENT: splats is not written. */
zoic_status zoic_splat_point(const zoic_camera *cam, const zoic_vec3 *Po, const zoic_pupil_bounds *bounds, uint32_t m,
                             const float *u /* m x 2 */, zoic_splat *splats /* m */);
zoic_status zoic_splat_point_spectral(const zoic_camera *cam, const zoic_vec3 *Po, const zoic_pupil_bounds *bounds, float wavelength_nm,
                                      uint32_t m, const float *u /* m x 2 */, zoic_splat *splats /* m */);

/* ---- trace-back transmittance: the Fresnel losses of backward lens paths (opt-in; csrc/traceback_throughput.hpp has the full definition) --
 * The backward calls above return geometry; the forward side's zoic_ray_transmittance_device says how much light the glass lets
 * through.  These calls give the same factor for a ray traced BACK, so that a light tracer, a splatter or a bidirectional integrator
 * weights both directions by the same lens: T = the product over the interfaces, front to rear, of the unpolarised Fresnel
 * transmittance of each, bare or with the interface's quarter-wave film (zoic_camera_set_coatings), at the ray's wavelength (the d-line
 * forms: 587.5618 nm), from the cosines and indices of the trace-back's own path.  No absorption.
 *   T          a traced ray (ZOIC_TRACED_BACK): a number in (0, 1].  Anything else -- every refusal reason, a wavelength outside
 *              [360, 830] nm or NaN -- gets +0.0.  THINLENS with depth of field: 1.0 where traced.  NONE, THINLENS without: +0.0.
 *   Ps, flags  the bits of the spectral trace-back call for every input (the d-line forms: of the d-line call); T rides along.
 *   Reciprocal the T of a forward record traced back equals zoic_ray_transmittance_device's T of that record, to rounding.
 *   Splat side the T of the very rays the two device splat calls trace (same point, bounds record, m and u): multiply a splat's weight
 *              by it.  A point with an empty box (ZOIC_SPLAT_NO_BOX) gets +0.0.
 * The films and the dispersion are read at the call: a zoic_camera_set_coatings or zoic_camera_set_abbe_numbers change needs no update.
 * The device calls and the host calls give the same bits for the same item in every precision mode.
 * Arguments, error codes, alignment, stream semantics and the threading contract: the ray side as the spectral trace-back device call,
 * the splat side as the spectral splat device call, except that d_screen and d_flags may both be NULL.  d_transmittance: floats, device
 * memory, 4-byte aligned.  n = 0 returns ZOIC_OK; m = 0 with n > 0 is ZOIC_ERR_INVALID_ARGUMENT; ZOIC_ERR_NO_DEVICE on a tables-only
 * camera.  No output is written on an argument error; no counter and no retry stream is touched. */
zoic_status zoic_trace_back_transmittance_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays, float *d_transmittance /* n */,
                                                 float *d_screen /* n x 2, may be NULL */, uint32_t *d_flags /* may be NULL */, void *stream);
zoic_status zoic_trace_back_transmittance_spectral_device(zoic_camera *cam, uint64_t n, const zoic_ray *d_rays,
                                                          const float *d_wavelengths /* n */, float *d_transmittance /* n */,
                                                          float *d_screen /* n x 2, may be NULL */, uint32_t *d_flags /* may be NULL */,
                                                          void *stream);
zoic_status zoic_splat_transmittance_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */,
                                            const zoic_pupil_bounds *d_bounds /* n */, uint32_t m, const float *d_u /* n x m x 2 */,
                                            float *d_transmittance /* n x m */, void *stream);
zoic_status zoic_splat_transmittance_spectral_device(zoic_camera *cam, uint64_t n, const float *d_points /* n x 3 */,
                                                     const zoic_pupil_bounds *d_bounds /* n */, const float *d_wavelengths /* n */, uint32_t m,
                                                     const float *d_u /* n x m x 2 */, float *d_transmittance /* n x m */, void *stream);
/* The host build of the same code for one ray, and for one point and its m aims (works on a ZOIC_DEVICE_NONE camera).  u and T of the
 * splat forms: host memory, 4-byte aligned; m = 0, a NULL pointer and a misaligned u or T are ZOIC_ERR_INVALID_ARGUMENT: T is not written. */
zoic_status zoic_trace_back_ray_transmittance(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir,
                                              float *Ps /* [2], may be NULL */, uint32_t *flags /* may be NULL */, float *T);
zoic_status zoic_trace_back_ray_transmittance_spectral(const zoic_camera *cam, const zoic_vec3 *origin, const zoic_vec3 *dir,
                                                       float wavelength_nm, float *Ps /* [2], may be NULL */,
                                                       uint32_t *flags /* may be NULL */, float *T);
zoic_status zoic_splat_point_transmittance(const zoic_camera *cam, const zoic_vec3 *Po, const zoic_pupil_bounds *bounds, uint32_t m,
                                           const float *u /* m x 2 */, float *T /* m */);
zoic_status zoic_splat_point_transmittance_spectral(const zoic_camera *cam, const zoic_vec3 *Po, const zoic_pupil_bounds *bounds,
                                                    float wavelength_nm, uint32_t m, const float *u /* m x 2 */, float *T /* m */);

/* Page-locked host memory for the buffers of zoic_create_rays_host: with pinned samples/rays the call runs as a
 * three-stream pipeline (copy-in of piece k+2, trace of piece k+1 and copy-out of piece k at once) at PCIe rate.  zoic_host_register pins
 * memory the caller already owns (keep it registered across calls: registration costs more than one transfer). */
zoic_status zoic_host_alloc(size_t bytes, void **out);
void        zoic_host_free(void *p);
zoic_status zoic_host_register(void *p, size_t bytes);
zoic_status zoic_host_unregister(void *p);

/* synthetic sample generator used by bench/tests: pixel-jittered screen samples, uniform lens samples */
zoic_status zoic_generate_samples_device(zoic_camera *cam, uint64_t n, uint64_t ray_index_base, uint32_t width,
                                         uint32_t height, uint32_t spp, uint32_t seed, float *d_samples, void *stream);

/* ---- one frame over several devices of ONE process ---------------------------------------------
 * The reference is one process whose render threads all call camera_create_ray on one node (zoic.cpp:1752; lifetime
 * :1565-1572, :1723-1749).  A zoic_frame is that node spread over n HIP devices of the calling process: one zoic_camera per
 * device (identical tables: node_update is deterministic), the samples of a call split into contiguous ray-index slabs
 * (zoic_frame_slab: 256-ray tiles, sizes differ by at most one tile), every device renders its slab with
 * zoic_create_rays_device's kernels, and the finished rays are moved to the root device (devices[0]).  Retry streams are
 * keyed by the GLOBAL ray index (ray_index_base + i), so the frame equals the one-device result bit for bit however many
 * devices it is split over.  No collective library is involved: a slab is cut into chunks, chunk k travels to the root with
 * hipMemcpyPeerAsync on the sending device's copy stream (xGMI is point to point: every peer pushes over its own link)
 * while chunk k+1 is traced; chunks alternate between two compute streams so that one's drain runs under the next one's
 * trace.  The root's own slab is ONE launch straight into the output; with one device the call IS
 * zoic_create_rays_device.  The same device may be listed more than once (a 1-GPU box exercises every code path with
 * devices = {0, 0}).
 * Threading: zoic_frame_create / _update / _set_* / _destroy as the camera's node_* methods (one thread, nothing in flight);
 * zoic_frame_render_* from one thread at a time per frame (a frame owns its streams and staging buffers; render threads that
 * want concurrency create one frame each, or call zoic_create_rays_* on zoic_frame_camera(frame, i) directly). */
typedef struct zoic_frame zoic_frame;
typedef enum zoic_frame_layout {
    ZOIC_FRAME_RECORDS = 0, /* n zoic_ray records (32 B/ray, flag word included) */
    ZOIC_FRAME_PAYLOAD = 1, /* n rows of 7 f32: ox oy oz dx dy dz weight (28 B/ray, SURVEY 8e's gather; the flag word stays on
                               the device that traced the ray) */
    ZOIC_FRAME_PAYLOAD_SPARSE = 2, /* the same n rows on the root, but only the rays with weight != 0 are TRANSPORTED: a peer's chunk
                               travels as a 256-bit live mask per 256-ray tile + the compacted rows of its live rays and is expanded
                               on the root.  Rows of weight-0 rays arrive as seven zeros: their origin / direction (the reference's
                               partial state of the last try, zoic.cpp:1951-1961) and their try counts are NOT transported -- they stay
                               in the tracing device's records.  Rows of live rays are bit-identical to ZOIC_FRAME_PAYLOAD's.  A wide-open
                               PETZVAL frame (79 % weight 0) moves 4.5x fewer bytes into the root.  The size of a chunk is only known on
                               the device: zoic_frame_render_device reads one 4-byte count per chunk back before it queues the copy, so
                               with this layout the call returns when the last chunk has been TRACED (copies and expansions may still
                               be in flight behind root_stream); zoic_frame_get_lane_info::bytes_to_root says what moved */
    ZOIC_FRAME_PAYLOAD_AUTO = 3 /* ZOIC_FRAME_PAYLOAD or ZOIC_FRAME_PAYLOAD_SPARSE, chosen from the camera: the first AUTO render after a
                               zoic_frame_update gathers dense; the next one reads the frame's ray counters (one synchronisation, once per
                               update) and from then on the gather is SPARSE iff at least 25 % of the rays rendered since the update had
                               weight 0 -- a wide-open PETZVAL (79 %) yes, the double Gauss with its bokeh image (0.07 %) never: there the
                               sparse layout's count read-back and expansion pass cost more than its headers save.  Rows of live rays are
                               the same bits either way; rows of weight-0 rays follow the layout chosen (dense: the reference's partial
                               state; sparse: zeros).  zoic_frame_auto_layout says what was chosen. */
} zoic_frame_layout;
/* ZOIC_FRAME_PAYLOAD_AUTO's decision for the tables the frame holds: ZOIC_FRAME_PAYLOAD, ZOIC_FRAME_PAYLOAD_SPARSE, or -1 while
 * undecided (no AUTO render since the last update, or only one).  zero_weight_fraction (may be NULL): what it measured, -1 undecided. */
int zoic_frame_auto_layout(const zoic_frame *frame, double *zero_weight_fraction);

/* [begin, end) of device i's slab of an n-sample call over n_devices devices.  Pure arithmetic, callable without a device. */
zoic_status zoic_frame_slab(uint64_t n, int n_devices, int i, uint64_t *begin, uint64_t *end);
/* node_initialize for every device (zoic_camera_create each); devices[0] is the root.  Enables peer access root <-> peers. */
zoic_status zoic_frame_create(const int *devices, int n_devices, zoic_frame **out);
void        zoic_frame_destroy(zoic_frame *frame);          /* node_finish for every device; waits for queued work */
int         zoic_frame_device_count(const zoic_frame *frame);
zoic_camera *zoic_frame_camera(zoic_frame *frame, int i);   /* device i's camera (getters, counters, per-sample calls) */
/* the camera's setters and node_update, applied to every device's camera (first failure is returned) */
zoic_status zoic_frame_set_bokeh_image(zoic_frame *frame, int width, int height, int nchannels, const float *pixels);
zoic_status zoic_frame_set_lens_text(zoic_frame *frame, const char *text, size_t len);
zoic_status zoic_frame_set_precision(zoic_frame *frame, zoic_precision mode);
zoic_status zoic_frame_set_seed(zoic_frame *frame, uint32_t seed);
zoic_status zoic_frame_update(zoic_frame *frame, const zoic_params *p);
/* rays per chunk of a peer's slab (rounded down to 256-ray tiles); 0 = default: a quarter of a slab, at least 64 MB of payload.
 * A slab is never cut into more than 64 chunks: a smaller value is raised to what gives 64. */
zoic_status zoic_frame_set_chunk_rays(zoic_frame *frame, uint64_t rays);
/* camera_create_ray over n samples resident on the devices.
 *   d_samples : n_devices pointers; d_samples[i] = device i's slab, (end - begin) x (sx, sy, lensx, lensy) f32 in device i's
 *               memory, complete before the call.  NULL: the slabs zoic_frame_generate_samples produced for this (n, base).
 *   d_out     : root-device memory for n records / payload rows (16-byte aligned), in global ray order
 *   root_stream : a stream of the root device (NULL = its default stream).  The call is asynchronous; everything it queued is
 *               ordered before whatever is queued on root_stream afterwards, and behind what was queued on it before. */
zoic_status zoic_frame_render_device(zoic_frame *frame, uint64_t n, const float *const *d_samples, uint64_t ray_index_base,
                                     void *d_out, zoic_frame_layout layout, void *root_stream);
/* same without moving anything to the root: every device leaves its slab's records in its own memory (d_rays[i], or the
 * frame's own buffers when d_rays is NULL) -- the "compute only" leg of a scaling measurement */
zoic_status zoic_frame_render_local(zoic_frame *frame, uint64_t n, const float *const *d_samples, uint64_t ray_index_base,
                                    zoic_ray *const *d_rays);
/* host buffers: device i moves its slab in and out over ITS OWN PCIe link (zoic_create_rays_host per device, all at once);
 * nothing crosses xGMI.  Returns when h_rays is complete. */
zoic_status zoic_frame_render_host(zoic_frame *frame, uint64_t n, const float *h_samples, uint64_t ray_index_base, zoic_ray *h_rays);
/* synthetic samples of zoic_generate_samples_device, every device its own slab, into frame-owned buffers */
zoic_status zoic_frame_generate_samples(zoic_frame *frame, uint64_t n, uint64_t ray_index_base, uint32_t width, uint32_t height,
                                        uint32_t spp, uint32_t seed);
zoic_status zoic_frame_synchronize(zoic_frame *frame);      /* every stream of the frame, on every device */
/* What device i's lane did in the last zoic_frame_render_device call, and how it reaches the root: peer_access_* = 1 when
 * hipDeviceCanAccessPeer said yes AND hipDeviceEnablePeerAccess succeeded in that direction (0: hipMemcpyPeerAsync stages through
 * the host -- correct, slow; the root itself and a device listed twice report 1: no link involved). */
typedef struct zoic_frame_lane_info {
    int32_t device, peer_access_to_root, peer_access_from_root;
    uint32_t chunks;              /* sub-launches of the slab */
    uint64_t rays;                /* the slab */
    uint64_t bytes_to_root;       /* bytes the lane's copies moved into the root's memory (0 for the root's own slab) */
} zoic_frame_lane_info;
zoic_status zoic_frame_get_lane_info(const zoic_frame *frame, int i, zoic_frame_lane_info *out);
zoic_status zoic_frame_get_counters(zoic_frame *frame, zoic_counters *sum);   /* summed over the devices */

/* ---- statistics (node_finish prints them, zoic.cpp:1729-1732) ------------------------------ */
zoic_status zoic_camera_get_counters(zoic_camera *cam, zoic_counters *out); /* synchronises the device */
zoic_status zoic_camera_reset_counters(zoic_camera *cam);

/* ---- introspection of the precomputed tables (parity tests) -------------------------------- */
typedef struct zoic_lens_info {
    int32_t lensCount, apertureElement;
    float userApertureRadius, originShift, apertureDistance, focalLengthRatio;
    float tracedFocalLength[2];
    float fov, tan_fov, apertureRadius;            /* thin lens, zoic.cpp:1606-1608 */
    float curvature[ZOIC_MAX_LENS_SURFACES], thickness[ZOIC_MAX_LENS_SURFACES], ior[ZOIC_MAX_LENS_SURFACES],
          aperture[ZOIC_MAX_LENS_SURFACES], center[ZOIC_MAX_LENS_SURFACES];
    int32_t lutSize;
    float lutKey[ZOIC_LUT_ENTRIES];
    float lutMaxX[ZOIC_LUT_ENTRIES], lutMaxY[ZOIC_LUT_ENTRIES], lutMinX[ZOIC_LUT_ENTRIES], lutMinY[ZOIC_LUT_ENTRIES];
    int32_t bokehWidth, bokehHeight;
    int32_t fastRunsStrict; /* 1: this camera is outside the FAST modes' domain (see zoic_precision) and runs STRICT whatever the mode */
    uint32_t precomputeTIR; /* totalInternalReflection bumps of node_update's own traces (zoic.cpp:1135 ff.) that the camera's
                               counters currently include (0 after zoic_camera_reset_counters) */
} zoic_lens_info;
zoic_status zoic_camera_get_info(const zoic_camera *cam, zoic_lens_info *out);
/* copies of the bokeh CDF tables (bokehProbability, zoic.cpp:222-417); arrays sized by bokehWidth/Height */
zoic_status zoic_camera_get_bokeh_tables(const zoic_camera *cam, float *cdfRow, int32_t *rowIndices, float *cdfColumn,
                                         int32_t *columnIndices);

#ifdef __cplusplus
}
#endif
#endif /* ZOIC_AMD_H */

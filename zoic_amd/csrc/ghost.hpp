// ghost.hpp -- ghost rays (zoic_create_ghost_rays_device): the path light takes through the lens when it is reflected at one interface and
// again at another before it reaches the sensor -- the flare discs and the veiling glare that coatings exist to suppress -- with its
// Fresnel weight.  transmittance.hpp subtracts the reflected light; this follows it.
//
// Definition.  One ghost belongs to one start (o, d) -- the accepted try of a forward record, trace frame, sensor side -- one wavelength
// (nm, valid: spectral_valid) and one ordered pair of interfaces (a, b), trace-order indices (rear first), a > b.  By reversibility it is
// the path scene light takes when it reflects first at b, then at a, and then reaches the sensor.  Traced from the sensor it has three legs:
//   leg 0, travelling +z   refract at interfaces 0 ... a-1, reflect at a;
//   leg 1, travelling -z   refract at a-1 ... b+1, reflect at b (no refraction when a == b+1);
//   leg 2, travelling +z   refract at b+1 ... count-1 and leave through the front element.
// At every interface visit, in this order:
//   1. u.z must have the leg's sign (kGhostTurned otherwise); after the last interface it must still be > 0 (kGhostTurned there).
//   2. the vertex-side intersection with the interface's sphere, the cap the forward trace takes (zoic.cpp:986); a miss ends the ghost
//      (kGhostMiss).  As in the forward trace a negative path length is not refused.
//   3. x^2 + y^2 against Surface::housing2 (kGhostClipped); the stop's entry is min(housing, user aperture)^2, and a ghost that crosses
//      the stop up to three times is clipped each time.
//   4. refraction or reflection about the unit normal (c x, c y, 1 + c z) of the vertex form, oriented against the leg's direction.
//      The indices of both sides are spectral_ior on the dispersion table (two roundings each); n_i lies behind interface i, 1.0 in front
//      of the front element.  Refraction: eta = n_from / n_to (equal media: exactly 1), k2 = eta^2 cosi^2 + 1 - eta^2, total internal
//      reflection (k2 < 0) ends the ghost (kGhostTir).  Reflection: u' = u + 2 cosi n.
// Weight: the Fresnel throughput only.  The product of interface_transmittance(n_from, n_to, |cosi|, sqrt(k2), film ...) at every
// refraction between unequal media -- every crossing at its own angle, so the interfaces between b and a count three times -- times
// R_a R_b, R = 1 - interface_transmittance(...) with the incidence side as n_from, and R = 1.0 exactly where the reflection is total
// (k2 < 0).  Films are read per interface as the transmittance pass reads them.  The caller multiplies the main record's weight in.
// Where the two media of a or of b are equal at the wavelength (always so at the stop) there is nothing to reflect at: kGhostNoReflection
// (interface a on leg 0, else b on leg 1), decided before anything is traced.
// "No pair" (a = b = -1, host and tests only: the C-ABI does not offer it) is the plain refracting path through all interfaces with
// weight = prod T_i: it ties this arithmetic to the STRICT trace and to path_transmittance.
//
// Output: one 32-byte record per (sample, pair).  Traced: origin on the front interface and dir out into the scene in the frame of the
// forward records (the forward store's final flip, zoic.cpp:1960-1961), dir of unit length to rounding, weight in (0, 1], flag bit 0.
// Ended early: origin, dir and weight +0.0, bit 0 clear, bits 8-11 the reason, bits 16-21 the interface, bits 24-25 the leg.
// The reasons that are decided before the trace are tested in this order and carry interface 0, leg 0: kGhostModel (THINLENS / NONE: a
// lens without interfaces has no ghosts), kGhostInvalidPair (a <= b or an index past the lens), kGhostNoStart (the main record has
// weight 0), kGhostWavelength (outside [360, 830] or NaN); then kGhostNoReflection, then kGhostNonFinite (a NaN / inf start, d = 0; also a
// result that is not finite).
//
// Arithmetic.  As traceback.hpp and transmittance.hpp: f32, contraction off, only correctly rounded operations (+ - x /, explicit fmaf,
// tb_sqrt / tb_rcp), so the host build and the kernel give the same bits.  z is kept RELATIVE to the current vertex and every sphere is
// taken in its vertex form c (x^2+y^2+z^2) + 2z = 0 as tb_trace takes it: no cancellation of two |R|-sized terms, at the stop's |R| ~ 1e4
// either, so the table needs no FAST-domain condition.  tb_trace's step is written for a ray going -z; a +z leg is that step on the
// mirror image (z, u.z, c -> -z, -u.z, -c).  The state below is kept in the current leg's mirrored coordinates (zm, um) and mirrored at
// each reflection, so there is one step and the sign only enters the curvature.  The start arrives in the forward trace's absolute
// frame and is converted once with the vertices of backward_vertices.
//
// Host- and device-callable (ZOIC_HD): tests/test_ghost_cpu.py drives a host build against an f64 numpy restatement (tests/ghost_ref.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "coating_stack.hpp"
#include "traceback.hpp"
#include "transmittance.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr uint32_t kGhostTraced = 1u;
constexpr uint32_t kGhostReasonShift = 8u, kGhostInterfaceShift = 16u, kGhostLegShift = 24u;
enum : uint32_t { kGhostMiss = 1u, kGhostClipped = 2u, kGhostTir = 3u, kGhostTurned = 4u, kGhostNoReflection = 5u, kGhostNonFinite = 6u,
                  kGhostWavelength = 7u, kGhostNoStart = 8u, kGhostModel = 9u, kGhostInvalidPair = 10u };
constexpr int kGhostMaxPairs = 32;   // per call: the pairs travel in the kernel arguments

// One interface, trace order.
struct alignas(16) GhostSurface {
    float step;       // this vertex minus the vertex of interface i-1 (the one behind it); 0 for entry 0
    float curv;       // 1 / radius (the stop: 1 / its |R| ~ 1e4 sphere)
    float housing2;   // clip limit on x^2 + y^2 (== Surface::housing2)
    float pad;
};

// The geometry of a camera's lens, filled by the host at zoic_camera_update from the rows fill_traceback_table reads.
struct GhostTable {
    int32_t model;      // ZOIC_THINLENS 0, ZOIC_RAYTRACED 1, ZOIC_LENS_NONE 2
    int32_t count;      // interfaces
    float vtxRear;      // the vertex of interface 0, trace frame: the start's z is taken relative to it
    float vtxFront;     // the vertex of interface count-1: the record's origin is absolute again
    GhostSurface surf[kMaxSurfaces];
};

// What is read at the call: the dispersion (spectral.hpp) and the films (transmittance.hpp) of every interface, trace order
struct GhostMedia {
    float iorD[kMaxSurfaces];      // n_d
    float cauchyB[kMaxSurfaces];   // B (nm^2)
    float filmIndex[kMaxSurfaces];     // nc; 0: uncoated
    float filmLambda0[kMaxSurfaces];   // nm
};

struct GhostRay { float ox, oy, oz, dx, dy, dz, weight; uint32_t flags; };

ZOIC_HD uint32_t ghost_pack(int a, int b) { return static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 8); }

ZOIC_HD GhostRay ghost_end(uint32_t reason, int interface, int leg)
{
    return GhostRay{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                    (reason << kGhostReasonShift) | (static_cast<uint32_t>(interface) << kGhostInterfaceShift) |
                        (static_cast<uint32_t>(leg) << kGhostLegShift)};
}

// the two media of interface i at dl: lo behind it (towards the sensor), hi in front of it
template <class MP>
ZOIC_HD void ghost_media(MP M, int count, int i, float dl, float &lo, float &hi)
{
    lo = spectral_ior(M->iorD[i], M->cauchyB[i], dl);
    hi = (i + 1 < count) ? spectral_ior(M->iorD[i + 1], M->cauchyB[i + 1], dl) : 1.0f;
}

// The ghost of the pair (a, b), or with a = b = -1 the plain path, from the start (o, d) at lambda.  GP: pointer to the GhostTable; MP:
// `const GhostMedia *` on the host, a pointer into the kernel-argument segment on the device (ZOIC_SPEC_PIN).  The pair is wave-uniform
// on the device, so the whole interface sequence is, and every table index goes through tb_uniform.  KP: the coating policy
// (coating_stack.hpp): NoStacks, or a pointer to the camera's StackTable, whose layers a +z leg meets in the table's order and leg 1
// backwards.
template <class GP, class MP, class KP = NoStacks>
ZOIC_HD GhostRay ghost_trace(GP G, MP M, int a, int b, float lambda, V3 o, V3 d, KP K = KP{})
{
    if (G->model != 1) return ghost_end(kGhostModel, 0, 0);
    const int count = G->count;
    const bool plain = a == -1 && b == -1;
    if (!plain && !(b >= 0 && a > b && a < count)) return ghost_end(kGhostInvalidPair, 0, 0);
    if (!spectral_valid(lambda)) return ghost_end(kGhostWavelength, 0, 0);
    const float dl = spectral_dl(lambda);
    if (!plain) {
        float lo, hi;
        MP m = M;
        ZOIC_SPEC_PIN(m);
        ghost_media(m, count, tb_uniform(a), dl, lo, hi);
        if (lo == hi) return ghost_end(kGhostNoReflection, a, 0);
        ghost_media(m, count, tb_uniform(b), dl, lo, hi);
        if (lo == hi) return ghost_end(kGhostNoReflection, b, 1);
    }
    if (!tb_finite(o.x, o.y, o.z) || !tb_finite(d.x, d.y, d.z)) return ghost_end(kGhostNonFinite, 0, 0);
    const float dm = fmaxf(fabsf(d.x), fmaxf(fabsf(d.y), fabsf(d.z)));
    if (!(dm > 0.0f)) return ghost_end(kGhostNonFinite, 0, 0);
    // the unit direction, as tb_trace takes it (scaled by its largest component first)
    const float im = tb_rcp(dm);
    const float ax = d.x * im, ay = d.y * im, az = d.z * im;
    const float il = tb_rcp(tb_sqrt(fmaf(ax, ax, fmaf(ay, ay, az * az))));
    float ux = ax * il, uy = ay * il, um = -(az * il);   // leg 0 travels +z: mirrored
    if (!tb_finite(ux, uy, um)) return ghost_end(kGhostNonFinite, 0, 0);
    float x = o.x, y = o.y, zm = -(o.z - G->vtxRear);
    float w = 1.0f;
    int i = 0, leg = 0;
    for (;;) {
        const int ii = tb_uniform(i), lg = tb_uniform(leg);
        const bool plus = lg != 1;                                     // the leg travels +z
        const bool reflect = (lg == 0 && ii == a) || (lg == 1 && ii == b);
        const GhostSurface S = G->surf[ii];                            // the whole entry at once
        const float step = plus ? S.step : G->surf[ii + 1].step;       // (leg 1 comes from interface ii + 1 <= a)
        const float c = plus ? -S.curv : S.curv;
        if (!(um < 0.0f)) return ghost_end(kGhostTurned, ii, lg);
        const float zr = zm + step;
        // tb_trace's step: the vertex-side root of c t^2 + 2 B t + F = 0 for a ray going -z (of the mirror image on a +z leg)
        const float F = fmaf(c, fmaf(x, x, fmaf(y, y, zr * zr)), zr + zr);
        const float B = fmaf(c, fmaf(x, ux, fmaf(y, uy, zr * um)), um);
        const float disc = fmaf(-c, F, B * B);
        if (!(disc >= 0.0f)) return ghost_end(kGhostMiss, ii, lg);
        const float sq = tb_sqrt(disc);
        const bool near = B <= 0.0f;
        const float rden = tb_rcp(near ? B - sq : c);
        const float t = (near ? -F : -(B + sq)) * rden;
        const float hx = fmaf(t, ux, x), hy = fmaf(t, uy, y), hz = fmaf(t, um, zr);
        if (!(fmaf(hx, hx, hy * hy) <= S.housing2)) return ghost_end(hx == hx && hy == hy ? kGhostClipped : kGhostMiss, ii, lg);
        const float nx = c * hx, ny = c * hy, nz = fmaf(c, hz, 1.0f);   // unit on the sphere; against the ray
        const float cosi = -fmaf(ux, nx, fmaf(uy, ny, um * nz));
        MP m = M;   // a copy per interface: the pinned pointer is not carried round the loop (transmittance.hpp)
        ZOIC_SPEC_PIN(m);
        float lo, hi;
        ghost_media(m, count, ii, dl, lo, hi);
        const float nc = m->filmIndex[ii], lambda0 = m->filmLambda0[ii];
        const float nFrom = plus ? lo : hi, nTo = plus ? hi : lo;
        const float eta = nFrom / nTo, eta2 = eta * eta;
        const float k2 = fmaf(eta2, cosi * cosi, 1.0f - eta2);
        if (reflect) {
            float R = 1.0f;   // total reflection
            if (k2 >= 0.0f) R = 1.0f - coated_transmittance(K, ii, plus, nFrom, nTo, fabsf(cosi), tb_sqrt(k2), nc, lambda0, lambda);
            w = w * R;
            const float g = cosi + cosi;
            ux = fmaf(g, nx, ux); uy = fmaf(g, ny, uy);
            um = -fmaf(g, nz, um);   // mirrored: the next leg travels the other way
            x = hx; y = hy; zm = -hz;
            leg = lg + 1;
            i = (leg == 1) ? ii - 1 : ii + 1;
        } else {
            if (!(k2 >= 0.0f)) return ghost_end(kGhostTir, ii, lg);
            const float sk = tb_sqrt(k2);
            if (nFrom != nTo) w = w * coated_transmittance(K, ii, plus, nFrom, nTo, fabsf(cosi), sk, nc, lambda0, lambda);
            const float g = fmaf(eta, cosi, -sk);
            ux = fmaf(eta, ux, g * nx); uy = fmaf(eta, uy, g * ny); um = fmaf(eta, um, g * nz);
            x = hx; y = hy; zm = hz;
            i = plus ? ii + 1 : ii - 1;
        }
        if (i >= count) break;   // (only a +z leg gets here: leg 1 ends in the reflection at b >= 0)
    }
    const int lastLeg = tb_uniform(leg);
    if (!(um < 0.0f)) return ghost_end(kGhostTurned, count - 1, lastLeg);
    // absolute again, then the forward store's final flip: the record's origin is -(x, y, vtxFront - zm), its dir -(ux, uy, -um)
    const float z = G->vtxFront - zm;
    // every refraction and reflection keeps the length only as well as its hit lies on its sphere: unit length again, once
    const float rl = tb_rcp(tb_sqrt(fmaf(ux, ux, fmaf(uy, uy, um * um))));
    ux = ux * rl; uy = uy * rl; um = um * rl;
    if (!tb_finite(x, y, z) || !tb_finite(ux, uy, um) || !(fabsf(w) <= kTbMaxFloat)) return ghost_end(kGhostNonFinite, count - 1, lastLeg);
    return GhostRay{x * -1.0f, y * -1.0f, z * -1.0f, ux * -1.0f, uy * -1.0f, um, w, kGhostTraced};
}

// One column of the call: the pair as the C-ABI packs it (a | b << 8), and whether the sample has a start at all
template <class GP, class MP, class KP = NoStacks>
ZOIC_HD GhostRay ghost_record(GP G, MP M, uint32_t pair, bool haveStart, float lambda, V3 o, V3 d, KP K = KP{})
{
    if (G->model != 1) return ghost_end(kGhostModel, 0, 0);
    const int a = static_cast<int>(pair & 0xFFu), b = static_cast<int>((pair >> 8) & 0xFFu);
    if ((pair >> 16) != 0u || !(a > b && a < G->count)) return ghost_end(kGhostInvalidPair, 0, 0);
    if (!haveStart) return ghost_end(kGhostNoStart, 0, 0);
    return ghost_trace(G, M, a, b, lambda, o, d, K);
}

// Host: the table of a camera from its LensView (backward_tables.hpp), the rows and the validity conditions of
// fill_traceback_table.
inline void fill_ghost_table(GhostTable &G, const LensView &L)
{
    G = GhostTable{};
    G.model = L.model;
    if (L.model != 1) return;
    if (!L.rows_valid()) { G.model = 2; return; }
    const int count = L.count;
    G.count = count;
    float vtx[kMaxSurfaces];
    backward_vertices(count, L.thickness, vtx);
    G.vtxRear = vtx[0];
    G.vtxFront = vtx[count - 1];
    for (int i = 0; i < count; ++i) {
        GhostSurface &S = G.surf[i];
        S.step = (i == 0) ? 0.0f : static_cast<float>(static_cast<double>(vtx[i]) - static_cast<double>(vtx[i - 1]));
        S.curv = static_cast<float>(1.0 / static_cast<double>(L.radius[i]));
        S.housing2 = backward_housing2(L, i);
    }
}

// the same from flat arguments (backward_tables.hpp lens_view_of_rows)
inline void fill_ghost_table(GhostTable &G, int model, int count, const float *radius, const float *thickness, const float *aperture,
                             int apertureElement, float userApertureRadius)
{
    fill_ghost_table(G, lens_view_of_rows(model, 0.0f, count, radius, thickness, nullptr, aperture, apertureElement, userApertureRadius));
}

// ---- launcher (ghost.hip) ------------------------------------------------------------------------------------------------
// The records of launch_kolb_rays / launch_kolb_spectral (k == 1) -> n x p ghost records, sample-major.  pairs: p <= kGhostMaxPairs packed
// pairs (host).  d_table: the camera's GhostTable on the device (RAYTRACED; not read otherwise).  d_lambda: n f32 (nm) or nullptr: the
// d-line.  model: ZOIC_THINLENS (0), ZOIC_RAYTRACED (1) or ZOIC_LENS_NONE (2).  Nothing but d_out is written.
// d_stacks: the camera's StackTable on the device where an interface has a stack (the stack-aware kernel), nullptr otherwise.
int launch_ghost_rays(int model, const KolbTable &kolb, const GhostMedia &media, const BokehTables &bokeh, const GhostTable *d_table,
                      uint32_t p, const uint32_t *pairs, const float *d_samples, const float *d_lambda, const uint32_t *d_rng,
                      uint64_t rayBase, uint64_t n, const RayRecord *rays, RayRecord *d_out, void *stream,
                      const StackTable *d_stacks = nullptr);

}  // namespace zoic

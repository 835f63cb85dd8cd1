// pupil_bounds.hpp -- pupil bounds (zoic_pupil_bounds_device, zoic_pupil_bounds_point and their _spectral forms): for a scene point,
// how much of the lens it sees and how big its blur spot on the sensor is.  project_points answers for the chief ray of a point,
// trace_back for one given ray, trace_back_jacobian for the change of measure -- and each leaves the step before it, how lens points
// are drawn, to the caller.  A light tracer or a splatter that draws them from the whole front element loses almost every ray on a
// stopped-down or vignetted camera (kTbClipped at the stop).  The forward path has the exit-pupil LUT (lut_build.hip) for the mirror
// image of that problem; this is the backward path's counterpart, and only its deterministic half: no random number, no weighting
// policy.  Every output is a min, a max, a count or an OR, so the answer does not depend on the order of the reduction and the host
// and the device agree bit for bit.
//
// Definition.
//   Input      a scene point P in the frame of the records (the frame project_point takes), a lattice size G in {8, 16, 32}, and a
//              film window (sx0, sy0, sx1, sy1); "no window" is (-inf, -inf, +inf, +inf), which every finite Ps passes.
//   Aims       G x G points A on a plane across the axis, the cell centres of the square [-R, R]^2:
//                RAYTRACED          the front vertex plane, z = -T.zFront of the record frame, R = sqrt(surf[0].housing2)
//                THINLENS with DOF  the lens plane z = 0, R = sqrt(aperture2)
//              ax = float(2 ix + 1 - G) (R / G), ay likewise with iy; R / G is exact (G a power of two), so each coordinate is one
//              rounding, and never zero (2 ix + 1 - G is odd).  The aim index is a = iy G + ix.
//   Ray        origin = P, dir = P - A: three f32 subtractions.  It points into the scene, as the trace-back wants; starting at P
//              keeps the cap test meaningful for front elements that are concave towards the scene.
//   Passing    an aim passes if trace_back_ray (spectral: trace_back_ray_spectral at the point's wavelength) sets kTbTraced and
//              sx0 <= sx <= sx1 and sy0 <= sy <= sy1.  A NaN window bound passes nothing.
//   Record     48 bytes:
//                aim[4]     (ax min, ay min, ax max, ay max) over the passing aims, each side grown by one pitch 2 R / G and clamped
//                           to +-R
//                screen[4]  (sx min, sy min, sx max, sy max) over the passing aims, not grown: the box of the blur spot
//                count      the number of passing aims
//                lattice    G^2: count / lattice x 4 R^2 is the area of the pupil as seen from P
//                flags      bit 0: at least one aim passes; bits 16-31: the OR over the refused aims of 1 << (16 + reason), reason a
//                           kTb* code (traceback.hpp) and 0, i.e. bit 16, for an aim that traced back but landed outside the window
//                reserved   0
//              With no aim passing, aim and screen are all +0.
//   Wholesale  what the trace-back refuses for every ray -- lensModel NONE, a pinhole thin lens (kTbModel), a camera outside the
//              geometric domain (kTbOutsideDomain), a non-finite P (kTbNonFinite), a P behind the front cap (kTbAway), an invalid
//              wavelength (kTbWavelength) -- comes out as count = 0 with that reason's bit: every aim is refused for it.  No error.
//
// What the bounds are: statements about the LATTICE, not a guarantee about the pupil.  Every passing lattice aim lies inside `aim`,
// and growing the box by a pitch covers the pupil's edge wherever the pupil is at least a pitch wide there; a sliver of pupil thinner
// than a pitch can pass between the aims and lie outside the grown box (DESIGN 4.17 has the measured share).  Where the whole pupil
// is thinner than a pitch -- a front housing much larger than the entrance pupil, as on a fisheye -- no aim may pass at all, and
// count = 0 then says nothing about whether P sees the lens (the corpus table and the fall-backs).  `screen` is the box of
// the lattice aims' landing points, nothing more.  The caller draws in `aim` and still traces every ray back: a draw outside the true
// pupil is refused there, as before.
//
// Arithmetic.  The trace is trace_back_ray's, untouched.  On top of it: one tb_sqrt, one exact division by G, per aim two int -> f32
// conversions (exact), two multiplications and three subtractions, and comparisons.  The running minima and maxima are seeded with
// +-kTbMaxFloat and updated by select, on values that are never NaN (an aim is finite; Ps of a traced ray is finite and never -0), so
// the merge of two partial results is associative and commutative bit for bit: the kernel's cross-lane butterfly and the host's
// loop give the same record.
//
// Host- and device-callable (ZOIC_HD): tests/test_pupil_bounds_cpu.py drives the host build against a numpy restatement.
#pragma once
#include <cstdint>

#include "backward_spectral.hpp"
#include "traceback.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr uint32_t kPbSome = 1u;            // flag bit 0: at least one aim passes
constexpr uint32_t kPbReasonShift = 16u;    // flag bit 16 + reason: an aim was refused for `reason`; reason 0: outside the window
constexpr float kPbInf = __builtin_huge_valf();

// the record as it lies in memory (zoic_pupil_bounds): three 16-byte rows
struct alignas(16) PupilBounds {
    float aim[4];
    float screen[4];
    uint32_t count, lattice, flags, reserved;
};

// the film window; the default passes every finite Ps
struct PupilWindow {
    float sx0 = -kPbInf, sy0 = -kPbInf, sx1 = kPbInf, sy1 = kPbInf;
};

ZOIC_HD bool pupil_lattice_valid(int G) { return G == 8 || G == 16 || G == 32; }

// the plane and the square the aims lie in: z of the plane (record frame), R, and the half pitch R / G
struct PupilFrame {
    float z, R, h;
};

ZOIC_HD PupilFrame pupil_frame(const TraceBackTable &T, int G)
{
    const bool thin = T.model == 0;
    const float R = tb_sqrt(thin ? T.aperture2 : T.surf[0].housing2);
    return PupilFrame{thin ? 0.0f : -T.zFront, R, R / static_cast<float>(G)};
}

// the ten running values of a set of aims
struct PupilAcc {
    float axMin = kTbMaxFloat, ayMin = kTbMaxFloat, axMax = -kTbMaxFloat, ayMax = -kTbMaxFloat;
    float sxMin = kTbMaxFloat, syMin = kTbMaxFloat, sxMax = -kTbMaxFloat, syMax = -kTbMaxFloat;
    uint32_t count = 0u, reasons = 0u;
};

ZOIC_HD float pb_min(float a, float b) { return b < a ? b : a; }
ZOIC_HD float pb_max(float a, float b) { return b > a ? b : a; }

// the union of two sets of aims
ZOIC_HD void pupil_merge(PupilAcc &A, const PupilAcc &B)
{
    A.axMin = pb_min(A.axMin, B.axMin); A.ayMin = pb_min(A.ayMin, B.ayMin);
    A.axMax = pb_max(A.axMax, B.axMax); A.ayMax = pb_max(A.ayMax, B.ayMax);
    A.sxMin = pb_min(A.sxMin, B.sxMin); A.syMin = pb_min(A.syMin, B.syMin);
    A.sxMax = pb_max(A.sxMax, B.sxMax); A.syMax = pb_max(A.syMax, B.syMax);
    A.count += B.count;
    A.reasons |= B.reasons;
}

// Aim a of the G x G lattice (G = 1 << shift) from P = (px, py, pz): trace(ox, oy, oz, dx, dy, dz, sx, sy) is the trace-back of
// that ray (it returns the flag word).
template <class Trace>
ZOIC_HD void pupil_aim(PupilAcc &A, const PupilFrame &F, int shift, int a, float px, float py, float pz, const PupilWindow &W, Trace trace)
{
    const int G = 1 << shift;
    const int ix = a & (G - 1), iy = a >> shift;
    const float ax = static_cast<float>(2 * ix + 1 - G) * F.h, ay = static_cast<float>(2 * iy + 1 - G) * F.h;
    float sx, sy;
    const uint32_t f = trace(px, py, pz, px - ax, py - ay, pz - F.z, sx, sy);
    const bool traced = (f & kTbTraced) != 0u;
    const bool pass = traced && sx >= W.sx0 && sx <= W.sx1 && sy >= W.sy0 && sy <= W.sy1;
    const uint32_t reason = traced ? 0u : ((f >> kTbReasonShift) & 0xFu);
    A.reasons |= pass ? 0u : (1u << (kPbReasonShift + reason));
    A.count += pass ? 1u : 0u;
    A.axMin = pass ? pb_min(A.axMin, ax) : A.axMin; A.ayMin = pass ? pb_min(A.ayMin, ay) : A.ayMin;
    A.axMax = pass ? pb_max(A.axMax, ax) : A.axMax; A.ayMax = pass ? pb_max(A.ayMax, ay) : A.ayMax;
    A.sxMin = pass ? pb_min(A.sxMin, sx) : A.sxMin; A.syMin = pass ? pb_min(A.syMin, sy) : A.syMin;
    A.sxMax = pass ? pb_max(A.sxMax, sx) : A.sxMax; A.syMax = pass ? pb_max(A.syMax, sy) : A.syMax;
}

// the record of all G^2 aims: the aim box grown by a pitch and clamped
ZOIC_HD PupilBounds pupil_record(const PupilAcc &A, const PupilFrame &F, int shift)
{
    PupilBounds B{};
    B.lattice = 1u << (2 * shift);
    B.count = A.count;
    B.flags = A.reasons;
    if (A.count == 0u) return B;
    const float pitch = 2.0f * F.h;
    B.flags |= kPbSome;
    B.aim[0] = pb_max(A.axMin - pitch, -F.R); B.aim[1] = pb_max(A.ayMin - pitch, -F.R);
    B.aim[2] = pb_min(A.axMax + pitch, F.R);  B.aim[3] = pb_min(A.ayMax + pitch, F.R);
    B.screen[0] = A.sxMin; B.screen[1] = A.syMin; B.screen[2] = A.sxMax; B.screen[3] = A.syMax;
    return B;
}

ZOIC_HD int pupil_shift(int G) { return G == 8 ? 3 : G == 16 ? 4 : 5; }

// One point on the host (the kernel walks the same aims 64 at a time, pupil_bounds.hip).  G must be pupil_lattice_valid.
template <class Trace>
ZOIC_HD PupilBounds pupil_bounds_of(const TraceBackTable &T, int G, float px, float py, float pz, const PupilWindow &W, Trace trace)
{
    const int shift = pupil_shift(G);
    const PupilFrame F = pupil_frame(T, G);
    PupilAcc A;
    for (int a = 0; a < G * G; ++a) pupil_aim(A, F, shift, a, px, py, pz, W, trace);
    return pupil_record(A, F, shift);
}

ZOIC_HD PupilBounds pupil_bounds_point(const TraceBackTable &T, int G, float px, float py, float pz, const PupilWindow &W)
{
    return pupil_bounds_of(T, G, px, py, pz, W, [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray(T, ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

ZOIC_HD PupilBounds pupil_bounds_point_spectral(const TraceBackTable &T, const BackwardDispersion &D, float lambda, int G, float px, float py,
                                                float pz, const PupilWindow &W)
{
    return pupil_bounds_of(T, G, px, py, pz, W, [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy) {
        return trace_back_ray_spectral(T, D, lambda, ox, oy, oz, dx, dy, dz, sx, sy);
    });
}

// ---- launchers (pupil_bounds.hip) -------------------------------------------------------------------------------------------
// d_points = n x 3 floats (4-byte aligned), d_lambda = n f32 wavelengths (nm), d_bounds = n 48-byte records (16-byte aligned).
// G must be pupil_lattice_valid.  Asynchronous on `stream`.
int launch_pupil_bounds(const TraceBackTable &T, const float *d_points, uint64_t n, int G, const PupilWindow &W, void *d_bounds, void *stream);
int launch_pupil_bounds_spectral(const TraceBackTable &T, const BackwardDispersion &D, const float *d_points, const float *d_lambda, uint64_t n,
                                 int G, const PupilWindow &W, void *d_bounds, void *stream);

}  // namespace zoic

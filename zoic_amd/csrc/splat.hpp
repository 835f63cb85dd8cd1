// splat.hpp -- lens splats (zoic_splat_points_device, zoic_splat_point and their _spectral forms): a scene point through drawn aims in
// its pupil box to the screen, with the two measures a splatter weights by.  pupil_bounds.hpp is the deterministic half of "where on the
// lens should a scene point aim"; this is the other half, and it stays deterministic: the caller brings the numbers u in [0, 1)^2, as
// for zoic_amd.pupil_rays, and nothing is drawn here.  It replaces the chain pupil_rays (host) -> trace_back_jacobian (8 + 4 + 48 bytes
// written per ray) -> solid_angle_measure (host) by one call that keeps the four numbers a splatter uses: where the ray lands, and by
// how much a step on the lens, or a step of the direction, moves it.  No sampling policy, no weighting policy, no accumulation.
//
// Definition.  Per item: a scene point P (the frame of the records), its 48-byte pupil-bounds record B as zoic_pupil_bounds_device
// wrote it, u = (u0, u1), and in the spectral form the point's wavelength.
//   Empty box  B.count == 0 or (B.flags & kPbSome) == 0: nothing is traced; the record is all +0 but flags = kSpNoBox (bit 12, which
//              neither the trace-back's flag word -- bits 0, 2, 8-11, 16-21 -- nor the projection's -- bits 0-2, 8-11 -- uses).
//   Aim        tx = B.aim[2] - B.aim[0];  ax = B.aim[0] + u0 tx (a product, then a sum);  ax = ax < lo ? lo : ax;  ax = ax > hi ? hi : ax
//              with lo = B.aim[0], hi = B.aim[2]; ay likewise from B.aim[1], B.aim[3] and u1.  These are pupil_rays' operations bit for
//              bit.  The two selects keep a NaN: a NaN u (or a NaN box) gives a NaN aim, which the trace refuses as kTbNonFinite.  u
//              outside [0, 1) lands on the box's edge.  The aim lies on the plane z = pupil_frame(T, .).z: -T.zFront (RAYTRACED), 0
//              (THINLENS).
//   Ray        origin = P, dir = P - A: three subtractions.  Traced by trace_back_ray_jacobian (spectral:
//              trace_back_ray_jacobian_spectral), untouched: sx, sy and the flag word are that call's bits.
//   Measures   written for a traced ray (kTbTraced), +0 otherwise; with J the trace's 2 x 6 Jacobian (row-major, J[3..5] = d sx/d dir,
//              J[9..11] = d sy/d dir):
//                area   = J[3] J[10] - J[4] J[9]: two products and a difference.  det d(sx, sy)/d(ax, ay) at fixed P: dir = P - A, so
//                         the derivative with respect to the aim is -J_d[:, 0:2], and the two signs cancel in the determinant.  Screen
//                         area per cm^2 of the aims' plane.
//                angle  = (area (r2 r)) / dz with r2 = (dx dx + dy dy) + dz dz, r = tb_sqrt(r2), dz of dir as given (negative for a
//                         traced ray), the quotient by div_rn.  dPs/d(omega), the value of solid_angle_measure(J, dir):  with a, b the
//                         rows of J_d, that measure is (a x b) . dir |dir|.  a . dir = b . dir = 0 (scaling dir moves nothing), so
//                         a x b is parallel to dir: (a x b) = k dir.  Its z component is a_x b_y - a_y b_x = area, so k = area / dz and
//                         (a x b) = (area / dz) dir.  Then (a x b) . dir |dir| = (area / dz) r2 r.
//              An entry that is not a number is written as the one quiet NaN (tbj_number), and so is a NaN ax or ay.
//   Record     32 bytes: sx, sy, ax, ay, area, angle, flags, reserved (= 0).  ax, ay are written for every record that was traced or
//              refused by the trace, and are +0 for kSpNoBox.
//   m          m >= 1 aims per point: splat i = p m + j (point-major) takes point p, record B[p], u[2 i], u[2 i + 1].
//
// Arithmetic.  As traceback_jacobian.hpp: contraction off, tb_sqrt and div_rn only.  On top of the trace, per splat: for the aim 2
// differences, 2 products, 2 sums and 4 selects; 3 differences for dir; 2 products and a difference for area; 3 products, 2 sums, a
// root, 2 products and a quotient for angle.  Each is one correctly rounded f32 operation on the host and on the device, none is fused,
// so a numpy float32 restatement (tests/splat_ref.py) gives the same bits.
//
// Host- and device-callable (ZOIC_HD): tests/test_splats_cpu.py drives the host build against that restatement.
#pragma once
#include <cstdint>

#include "pupil_bounds.hpp"
#include "traceback_jacobian.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr uint32_t kSpNoBox = 1u << 12;   // the point's pupil box is empty: nothing was traced

// the record as it lies in memory (zoic_splat): two 16-byte rows
struct alignas(16) Splat {
    float sx, sy, ax, ay;
    float area, angle;
    uint32_t flags, reserved;
};

// one coordinate of the aim: lo + u (hi - lo), clamped by two selects that keep a NaN
ZOIC_HD float splat_aim(float lo, float hi, float u)
{
    const float t = hi - lo;
    const float p = u * t;
    float a = lo + p;
    a = a < lo ? lo : a;
    a = a > hi ? hi : a;
    return a;
}

// One splat: the point (px, py, pz), its box (lo x, lo y, hi x, hi y) with the record's count and flags, (u0, u1), and the aims' plane
// z.  trace(ox, oy, oz, dx, dy, dz, sx, sy, J) is the trace-back with its Jacobian (it returns the flag word).
template <class Trace>
ZOIC_HD Splat splat_of(float z, float px, float py, float pz, float lox, float loy, float hix, float hiy, uint32_t count, uint32_t boxFlags,
                       float u0, float u1, Trace trace)
{
    Splat S{};
    if (count == 0u || (boxFlags & kPbSome) == 0u) {
        S.flags = kSpNoBox;
        return S;
    }
    const float ax = splat_aim(lox, hix, u0), ay = splat_aim(loy, hiy, u1);
    const float dx = px - ax, dy = py - ay, dz = pz - z;
    float J[12];
    const uint32_t f = trace(px, py, pz, dx, dy, dz, S.sx, S.sy, J);
    S.ax = tbj_number(ax);
    S.ay = tbj_number(ay);
    S.flags = f;
    if ((f & kTbTraced) != 0u) {
        const float p0 = J[3] * J[10], p1 = J[4] * J[9];
        const float area = p0 - p1;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float r2 = (xx + yy) + zz;
        const float r = tb_sqrt(r2);
        const float r3 = r2 * r;
        const float num = area * r3;
        S.area = tbj_number(area);
        S.angle = tbj_number(div_rn(num, dz));
    }
    return S;
}

ZOIC_HD float splat_plane(const TraceBackTable &T) { return pupil_frame(T, 1).z; }

// the d-line splat of one item
ZOIC_HD Splat splat_point(const TraceBackTable &T, float px, float py, float pz, const PupilBounds &B, float u0, float u1)
{
    return splat_of(splat_plane(T), px, py, pz, B.aim[0], B.aim[1], B.aim[2], B.aim[3], B.count, B.flags, u0, u1,
                    [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, float *J) {
                        return trace_back_ray_jacobian(T, ox, oy, oz, dx, dy, dz, sx, sy, J);
                    });
}

// the same at the point's wavelength (nm)
ZOIC_HD Splat splat_point_spectral(const TraceBackTable &T, const BackwardDispersion &D, float lambda, float px, float py, float pz,
                                   const PupilBounds &B, float u0, float u1)
{
    return splat_of(splat_plane(T), px, py, pz, B.aim[0], B.aim[1], B.aim[2], B.aim[3], B.count, B.flags, u0, u1,
                    [&](float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, float *J) {
                        return trace_back_ray_jacobian_spectral(T, D, lambda, ox, oy, oz, dx, dy, dz, sx, sy, J);
                    });
}

// ---- launchers (splat.hip) ------------------------------------------------------------------------------------------------------
// d_points = n x 3 floats (4-byte aligned), d_bounds = n 48-byte pupil-bounds records (16-byte aligned), d_u = n x m x 2 floats
// (8-byte aligned), d_lambda = n f32 wavelengths (nm), d_splats = n x m 32-byte records (16-byte aligned).  m >= 1 and n m < 2^58.
// Asynchronous on `stream`.
int launch_splat_points(const TraceBackTable &T, const float *d_points, const void *d_bounds, uint64_t n, uint32_t m, const float *d_u,
                        void *d_splats, void *stream);
int launch_splat_points_spectral(const TraceBackTable &T, const BackwardDispersion &D, const float *d_points, const void *d_bounds,
                                 const float *d_lambda, uint64_t n, uint32_t m, const float *d_u, void *d_splats, void *stream);

}  // namespace zoic

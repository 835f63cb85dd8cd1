// traceback_jacobian.hpp -- the Jacobian of the trace-back (zoic_trace_back_jacobian_device, zoic_trace_back_ray_jacobian and their
// spectral forms): besides the screen sample Ps = (sx, sy) on which a camera ray lands (traceback.hpp), how Ps moves with the ray.
// A light tracer, a splatter or a bidirectional integrator that connects a scene point to a lens point needs the change of measure
// from that ray to the screen: |det dPs/d(omega)| at a fixed origin for a splat, dPs/d(origin) for a connection to a point on the
// front element.  Finite differences of the trace-back cost 12 more traces per ray, are good to about three digits in f32 and break
// next to a clip edge; the tangents below ride along with the one trace.
//
// Definition.  For a ray that trace_back_ray traces back (flag bit 0 set),
//       J = d(sx, sy) / d(origin.x, origin.y, origin.z, dir.x, dir.y, dir.z)
//   Layout     2 x 6, row-major: the six derivatives of sx, then the six of sy.  J_o = the columns 0-2, J_d = the columns 3-5.
//   dir        is differentiated AS GIVEN, at any length.
//   Map        J is the derivative of the exact map traceback.hpp defines: the move to the front vertex plane, the normalisation,
//              then at every interface the vertex-side hit, the normal and Snell, and finally the sensor plane.
//   Identities J_o . dir = 0 and J_d . dir = 0: moving the origin along the line changes nothing, scaling dir changes nothing.
//   No part    the cap test, the LUT flag and the clip decisions have no derivative.
//   THINLENS   (with useDof) in closed form.  With tau = -(oz + fd) / dz and I = 1 / (fd tan_fov):
//              sx = (ox + tau dx) I;  d sx/d ox = I;  d sx/d oz = -(dx / dz) I;  d sx/d dx = tau I;  d sx/d dz = (oz + fd) dx / dz^2 I
//              = -tau (dx / dz) I;  d sx/d oy = d sx/d dy = 0; likewise sy with y for x.
//   Wavelength The spectral form holds the wavelength fixed: eta carries no tangent.  An invalid wavelength gives kTbWavelength.
//   Not traced A ray that is not traced back gets Ps = (+0, +0) and twelve +0.0.
//   Overflow   J is not clipped: for a ray of an extreme scale an entry may be +-inf; an entry that is not a number is written as the
//              one quiet NaN 0x7fc00000 (a NaN's sign and payload are the only bits the host and the device may disagree on).
//
// Ps and flags are trace_back_ray's bit for bit, for every input, by construction: both run the one primal sequence, traceback.hpp's
// tb_trace, and the tangents below only ride along with it (its Tangents parameter) -- they read the trace's values at five fixed
// points and write J, never a value the trace reads.
//
// Tangents.  The rays through the lens are a 4-dimensional manifold, and the start step is analytic, so FOUR tangents are carried
// through the interfaces (24 live registers, not 36) and composed with the start step's 4 x 6 at the end:
//   Start      p = (x, y) in the front vertex plane, u = dir / |dir|.  x = s dx - ox, y = s dy - oy with s = (oz + zFront) / dz, and z
//              stays 0 whatever the ray (its derivative is exactly 0).  The four seeds are a unit step of x, a unit step of y, and
//              u turned towards e1 and towards e2, (e1, e2) an orthonormal basis of the plane across u (the branch of Duff et al.,
//              "Building an orthonormal basis, revisited", JCGT 2017, for u.z < 0: 1 - u.z >= 1, no cancellation at any angle).
//              d(x, y)/d origin = [-1 0 dx/dz; 0 -1 dy/dz];  d(x, y)/d dir = s [1 0 -dx/dz; 0 1 -dy/dz];
//              du/d dir = (I - u u^T) / |dir|, whose coordinates in (e1, e2) are e1^T / |dir| and e2^T / |dir|.
//   Interface  Igehy's transfer and refraction (record_pass.hpp applies them in the forward direction), per tangent:
//              dt = -n . (dp + t du) / (n . u);  dh = dp + t du + u dt;  dn = c dh;  dcos = -(du . n + u . dn);
//              d sqrt(k2) = eta^2 cos dcos / sqrt(k2), so dg = dcos (eta - eta^2 cos / sqrt(k2)) = dcos (-eta g / sqrt(k2));
//              du' = eta du + dg n + g dn;  dz follows z + S.dz unchanged.
//   Sensor     dt = -(dz + t du.z) / u.z;  dP = dp + t du + u dt, times 1 / halfSensor.
//
// Arithmetic.  As traceback.hpp: f32 with explicit fmaf and contraction off; tb_sqrt, tb_rcp and div_rn only; the same operations
// in every precision mode, so the host build and the kernel give the same bits for J too.
//
// Host- and device-callable (ZOIC_HD): tests/test_traceback_jacobian_cpu.py drives the host build against f64 central differences.
#pragma once
#include <cstdint>
#include <cstring>

#include "backward_spectral.hpp"
#include "traceback.hpp"

#pragma STDC FP_CONTRACT OFF

namespace zoic {

// one tangent of the ray's state: position (z relative to the current vertex) and unit direction
struct TbTangent {
    float x, y, z, ux, uy, uz;
};

ZOIC_HD float tbj_number(float v)
{
    if (v == v) return v;
    const uint32_t q = 0x7fc00000u;   // the one NaN both builds write
    float r;
    memcpy(&r, &q, sizeof r);
    return r;
}

ZOIC_HD void tbj_zero(float *J)
{
    for (int k = 0; k < 12; ++k) J[k] = 0.0f;
}

// The four tangents riding along with tb_trace (traceback.hpp's Tangents): the slopes of the line, the basis across u, and D[4].
struct TbFourTangents {
    float *J;
    float sxz, syz;                          // the line's slopes dx / dz, dy / dz
    float e1x, e1y, e1z, e2x, e2y, e2z;
    TbTangent D[4];

    ZOIC_HD void line(float dx, float dy, float idz) { sxz = dx * idz; syz = dy * idz; }

    // THINLENS, the closed form: tau = -(oz + fd) / dz
    ZOIC_HD void thin(const TraceBackTable &T, float s, float sf)
    {
        const float I = T.invFocalTan;
        const float tauI = (s + sf) * I;
        J[0] = I;                        J[7] = I;
        J[2] = tbj_number(-sxz * I);     J[8] = tbj_number(-syz * I);
        J[3] = tbj_number(tauI);         J[10] = tbj_number(tauI);
        J[5] = tbj_number(-tauI * sxz);  J[11] = tbj_number(-tauI * syz);
    }

    // the four seeds: x, y, and u towards e1, e2 (u.z < 0)
    ZOIC_HD void seed(float ux, float uy, float uz)
    {
        const float ba = tb_rcp(1.0f - uz), bb = ux * uy * ba;
        e1x = fmaf(-ux * ux, ba, 1.0f); e1y = -bb; e1z = ux;
        e2x = bb; e2y = fmaf(uy * uy, ba, -1.0f); e2z = -uy;
        D[0] = TbTangent{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        D[1] = TbTangent{0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        D[2] = TbTangent{0.0f, 0.0f, 0.0f, e1x, e1y, e1z};
        D[3] = TbTangent{0.0f, 0.0f, 0.0f, e2x, e2y, e2z};
    }

    // one interface, with the ray's direction u BEFORE the refraction
    ZOIC_HD void interface(float c, float t, float nx, float ny, float nz, float cosi, float eta, float sk, float g, float ux, float uy,
                           float uz)
    {
        const float icos = tb_rcp(cosi);                // n . u = -cosi
        const float gc = -(eta * g) * tb_rcp(sk);       // dg / dcos
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            TbTangent &d = D[k];
            const float wx = fmaf(t, d.ux, d.x), wy = fmaf(t, d.uy, d.y), wz = fmaf(t, d.uz, d.z);
            const float dt = fmaf(nx, wx, fmaf(ny, wy, nz * wz)) * icos;
            const float dhx = fmaf(ux, dt, wx), dhy = fmaf(uy, dt, wy), dhz = fmaf(uz, dt, wz);
            const float dnx = c * dhx, dny = c * dhy, dnz = c * dhz;
            const float dcos = -(fmaf(d.ux, nx, fmaf(d.uy, ny, d.uz * nz)) + fmaf(ux, dnx, fmaf(uy, dny, uz * dnz)));
            const float dg = dcos * gc;
            d.ux = fmaf(eta, d.ux, fmaf(dg, nx, g * dnx));
            d.uy = fmaf(eta, d.uy, fmaf(dg, ny, g * dny));
            d.uz = fmaf(eta, d.uz, fmaf(dg, nz, g * dnz));
            d.x = dhx; d.y = dhy; d.z = dhz;
        }
    }

    // the sensor plane: d(sx, sy) along each of the four tangents, then the start step's 4 x 6.  1 / |dir| = im il.
    ZOIC_HD void sensor(const TraceBackTable &T, float t, float iuz, float ux, float uy, float s, float im, float il)
    {
        float gx[4], gy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const TbTangent &d = D[k];
            const float dt = -fmaf(t, d.uz, d.z) * iuz;
            gx[k] = fmaf(ux, dt, fmaf(t, d.ux, d.x)) * T.invHalfSensor;
            gy[k] = fmaf(uy, dt, fmaf(t, d.uy, d.y)) * T.invHalfSensor;
        }
        const float kx = fmaf(gx[0], sxz, gx[1] * syz), ky = fmaf(gy[0], sxz, gy[1] * syz);   // d / d oz
        const float ax1 = gx[2] * il * im, ax2 = gx[3] * il * im, ay1 = gy[2] * il * im, ay2 = gy[3] * il * im;
        J[0] = tbj_number(-gx[0]);
        J[1] = tbj_number(-gx[1]);
        J[2] = tbj_number(kx);
        J[3] = tbj_number(fmaf(s, gx[0], fmaf(ax1, e1x, ax2 * e2x)));
        J[4] = tbj_number(fmaf(s, gx[1], fmaf(ax1, e1y, ax2 * e2y)));
        J[5] = tbj_number(fmaf(-s, kx, fmaf(ax1, e1z, ax2 * e2z)));
        J[6] = tbj_number(-gy[0]);
        J[7] = tbj_number(-gy[1]);
        J[8] = tbj_number(ky);
        J[9] = tbj_number(fmaf(s, gy[0], fmaf(ay1, e1x, ay2 * e2x)));
        J[10] = tbj_number(fmaf(s, gy[1], fmaf(ay1, e1y, ay2 * e2y)));
        J[11] = tbj_number(fmaf(-s, ky, fmaf(ay1, e1z, ay2 * e2z)));
    }
};

// the trace-back of one ray and its Jacobian: returns the flag word, writes sx, sy and J[12]
template <class Medium = TbDLine>
ZOIC_HD uint32_t trace_back_ray_jacobian(const TraceBackTable &T, float ox, float oy, float oz, float dx, float dy, float dz, float &sx,
                                         float &sy, float *J, Medium M = Medium())
{
    tbj_zero(J);
    TbFourTangents G;
    G.J = J;
    return tb_trace(T, ox, oy, oz, dx, dy, dz, sx, sy, M, G);
}

// the same at the ray's wavelength (nm), held fixed
ZOIC_HD uint32_t trace_back_ray_jacobian_spectral(const TraceBackTable &T, const BackwardDispersion &D, float lambda, float ox, float oy,
                                                  float oz, float dx, float dy, float dz, float &sx, float &sy, float *J)
{
    if (!spectral_valid(lambda)) {
        sx = 0.0f; sy = 0.0f;
        tbj_zero(J);
        return kTbWavelength << kTbReasonShift;
    }
    return trace_back_ray_jacobian(T, ox, oy, oz, dx, dy, dz, sx, sy, J, TbSpectral{D.med, spectral_dl(lambda), 1.0f});
}

// ---- launchers (traceback.hip) ----------------------------------------------------------------------------------
// As launch_trace_back / launch_trace_back_spectral, with d_jacobian = n x 12 floats (16-byte aligned).  Asynchronous on `stream`.
int launch_trace_back_jacobian(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian,
                               void *stream);
int launch_trace_back_jacobian_spectral(const TraceBackTable &T, const BackwardDispersion &D, const void *d_rays, const float *d_lambda,
                                        uint64_t n, float *d_screen, uint32_t *d_flags, float *d_jacobian, void *stream);

}  // namespace zoic

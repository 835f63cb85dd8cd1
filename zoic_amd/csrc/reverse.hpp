// reverse.hpp -- reverse projection (zoic_project_points_device, zoic_project_point, the opt-in zoic_camera_reverse_ray): the screen
// sample Ps = (sx, sy) whose ray passes through a given point Po.  The reference leaves camera_reverse_ray a stub that returns
// false (zoic.cpp:1992-1995); this is the map it would have answered.
//
// Definition.
//   Frame      Po is given in the frame of the records the forward calls write (zoic_ray origin and direction after the
//              reference's final flips).  THINLENS: dir.z *= -1 (zoic.cpp:1845).  RAYTRACED: origin and direction negated
//              (zoic.cpp:1960-1961), so the trace-frame point is Q = -Po.  Ps is the sample the forward calls would take: for a
//              Kolb lens the sensor point (sx halfSensor, sy halfSensor, originShift) -- sy scaled by the WIDTH too, zoic.cpp:1853-1854.
//   THINLENS   Ps is the sample whose lens-centre ray passes through Po.  That ray runs from the origin towards
//              (sx tanFov, sy tanFov, -1), so sx = Po.x / (-Po.z) / tanFov, sy likewise; projected only if Po.z < 0.  Depth of
//              field, optical vignetting and the bokeh image do not move the chief ray.
//   RAYTRACED  Ps is the sensor point of the CHIEF ray: the ray through Q and through the centre of the aperture stop, refracted at
//              every interface.  The lens is rotationally symmetric, so that ray lies in the meridional plane of Q and the search
//              is one-dimensional, in (r, z):
//                - every sphere has its vertex at computeLensCenters' summed thickness (zoic.cpp:963-969; the reference's centre
//                  is that vertex minus the radius, rounded to f32) and the trace takes its vertex-side intersection (of the two
//                  roots the one with the larger sgn(R) z, as zoic.cpp:986 picks it);
//                - the stop is the plane through its vertex (the reference traces it as a sphere of |R| ~ 1e4: the same point
//                  on the axis);
//                - where several roots exist, the one continuous with the paraxial solution, that is with the axis: the search
//                  keeps the axis ray as one end of its bracket;
//                - a point on the axis gives exactly (+0, +0).
//              Cameras outside the geometric FAST domain (negative focal-length rescale, or the sensor in front of the rear
//              vertex: the geometric half of zoic_lens_info::fastRunsStrict) and lens model NONE project no point.
//   Flags      bit 0  projected: Ps is written (the enabled zoic_camera_reverse_ray returns 1)
//              bit 1  the chief ray is clipped by some element's housing (Ps is still the chief ray's)
//              bit 2  the sensor radius lies beyond the exit-pupil LUT's last key (forward rays there carry zoic_ray flag bit 6)
//              bits 8-11, when bit 0 is clear: kRevBehind, kRevNoRoot, kRevNonFinite, kRevModelNone, kRevOutsideDomain.
//              A point that is not projected gets Ps = (+0, +0).
//
// Search (RAYTRACED).  The unknown is s, the sine of the chief ray's angle to the axis where it leaves the stop's centre towards the
// front.  G(s) = the signed distance of Q from the line of that ray after the front group, traced with its tangent dG/ds carried
// alongside (the intersection, normal and Snell terms differentiated in closed form).  The axis ray (s = 0) always gets out and has
// G < 0 for a point off the axis: it is one end of the bracket.  First guess: the paraxial chief ray through the entrance pupil's
// centre.  Safeguarded Newton: a step whose ray does not get out is halved back towards the last s whose ray did; once G has changed
// sign the iterate stays inside the bracket (bisection otherwise); at most kRevMaxIter evaluations.  Converged: |G| <= 2^-20 x
// max(|Q - P|, the front element's radius), P the exit point -- then one more Newton step, unchecked -- or a step below an ulp of s.
// The chief ray is then traced from the stop's centre through the back group to the sensor plane (and once more through the front
// group, without tangent, for the clip flag).
//
// Arithmetic.  f32 with explicit fmaf and contraction off, and correctly rounded square roots and reciprocals (device: the
// sequences of exact_math.hpp; host: sqrtf and 1.0f / x), so the host build (zoic_project_point) and the device kernel
// (reverse.hip) give the same bits in every precision mode.  The trace keeps z RELATIVE to the current vertex (a few cm at most),
// never absolute, and takes each sphere in its vertex form (Spencer and Murty: no cancellation of two |R|-sized terms, a plane for
// R = inf); no ray starts at Q, so a point 1e4 cm away costs no precision.
//
// Host- and device-callable (ZOIC_HD): tests/test_reverse_cpu.py drives the host build against an f64 restatement.
#pragma once
#include <cmath>
#include <cstdint>

#include "backward_tables.hpp"
#include "tables.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#include "exact_math.hpp"
#endif

#pragma STDC FP_CONTRACT OFF

namespace zoic {

constexpr uint32_t kRevProjected = 1u, kRevClipped = 2u, kRevPastLut = 4u;
constexpr uint32_t kRevReasonShift = 8u;
enum : uint32_t { kRevBehind = 1u, kRevNoRoot = 2u, kRevNonFinite = 3u, kRevModelNone = 4u, kRevOutsideDomain = 5u,
                  kRevWavelength = 6u };   // (kRevWavelength: the spectral calls only, backward_spectral.hpp)
constexpr int kRevMaxIter = 12;
constexpr float kRevTol = 9.5367431640625e-07f;   // 2^-20: the distance by which the exit ray may miss the point, per max(|Q - P|, front radius)

#if defined(__HIP_DEVICE_COMPILE__)
ZOIC_HD float rev_sqrt(float x) { return sqrt_rn(x); }
ZOIC_HD float rev_rcp(float x) { return rcp_rn(x); }
#else
ZOIC_HD float rev_sqrt(float x) { return sqrtf(x); }
ZOIC_HD float rev_rcp(float x) { return 1.0f / x; }
#endif

// One interface, front-to-back order.
struct RevSurface {
    float dz;         // vertex of the previous interface (front-to-back) minus this vertex: the z step between their frames
    float curv;       // 1 / radius; 0 for the stop (a plane)
    float etaF;       // towards the front (+z): ior of the rear-side medium / ior of the front-side medium
    float etaR;       // towards the rear (-z): its inverse, rounded once
    float housing2;   // clip limit on r^2 (== Surface::housing2: the stop's holds min(housing, user aperture)^2)
};

// Filled by the host at zoic_camera_update; a kernel argument by value (wave-uniform: scalar loads).
struct ReverseTable {
    int32_t model;        // ZOIC_THINLENS 0, ZOIC_RAYTRACED 1, ZOIC_LENS_NONE 2
    int32_t domain;       // RAYTRACED: 1 inside the geometric domain, 0 outside (every point reported kRevOutsideDomain)
    int32_t count;        // interfaces
    int32_t stop;         // index of the stop, front-to-back
    int32_t useLUT;       // kolbSamplingLUT: flag bit 2 is set against lutSize
    int32_t lutSize;
    float tanFov;         // THINLENS (zoic.cpp:1607)
    float halfSensor;     // sensorWidth * 0.5 (zoic.cpp:1853-1854)
    float invHalfSensor;  // 1 / halfSensor
    float sensorZ;        // the sensor plane relative to the rear vertex: originShift - vertex(rear)
    float zFront;         // the front vertex, trace frame
    float zPupil;         // the paraxial entrance pupil (trace frame)
    float pupilSlope;     // paraxial slope at the stop per slope in object space (1 / the pupil's angular magnification)
    float frontRadius;    // the front element's housing radius: the length below which the search's tolerance stops shrinking
    float pad[2];
    RevSurface surf[kMaxSurfaces];
};

struct RevRay { float x, z, ur, uz; };   // meridional state: height, z relative to the current vertex, unit direction

// One interface: intersection, housing clip, refraction, for a ray travelling towards +z (FWD) or -z.  The sphere in its vertex
// form, c (x^2 + z^2) + 2 z = 0 (z relative to the vertex, c = 1 / R): the root on the vertex side (zoic.cpp:986, the larger
// sgn(R) z of the two) in the form without cancellation.  `shift` moves z into this interface's frame.  With TAN the tangent
// (d/ds of every state component) is carried alongside.  M gives the ratio of the two media in the direction of travel (RevDLine:
// S.etaF / S.etaR).  Returns false on a sphere miss or total internal reflection.
template <bool TAN, bool FWD, class Medium>
ZOIC_HD bool rev_interface(const RevSurface &S, Medium &M, int j, float shift, RevRay &r, RevRay &d, bool &clipped)
{
    const float c = S.curv;
    const float zr = r.z + shift;
    const float x = r.x;
    const float F = fmaf(c, fmaf(x, x, zr * zr), zr + zr);
    const float B = fmaf(c, fmaf(x, r.ur, zr * r.uz), r.uz);
    const float disc = fmaf(-c, F, B * B);
    if (!(disc >= 0.0f)) return false;
    const float sq = rev_sqrt(disc);
    // FWD: -F / (B + sq) while B >= 0, (sq - B) / c beyond;  towards -z: -F / (B - sq) while B <= 0, (-B - sq) / c beyond
    const bool near = FWD ? B >= 0.0f : B <= 0.0f;
    const float den = near ? (FWD ? B + sq : B - sq) : c;
    const float rden = rev_rcp(den);
    const float t = (near ? -F : (FWD ? sq - B : -(B + sq))) * rden;
    const float hx = fmaf(t, r.ur, x), hz = fmaf(t, r.uz, zr);
    if (hx * hx > S.housing2) clipped = true;
    // the unit normal on the sphere, (c x, 1 + c z), turned against the ray
    const float sg = FWD ? -1.0f : 1.0f;
    const float nx = sg * (c * hx), nz = sg * fmaf(c, hz, 1.0f);
    const float cosi = -fmaf(r.ur, nx, r.uz * nz);
    const float eta = FWD ? M.eta_front(j, S) : M.eta_rear(j, S), eta2 = eta * eta;
    const float k2 = fmaf(eta2, cosi * cosi, 1.0f - eta2);
    if (!(k2 >= 0.0f)) return false;
    const float sk = rev_sqrt(k2);
    const float g = fmaf(eta, cosi, -sk);
    if constexpr (TAN) {
        const float dF = 2.0f * fmaf(c, fmaf(x, d.x, zr * d.z), d.z);
        const float dB = fmaf(c, fmaf(d.x, r.ur, fmaf(x, d.ur, fmaf(d.z, r.uz, zr * d.uz))), d.uz);
        const float dDisc = fmaf(2.0f * B, dB, -c * dF);
        const float dsq = dDisc * 0.5f * rev_rcp(sq);
        const float dt = near ? -fmaf(t, FWD ? dB + dsq : dB - dsq, dF) * rden : (FWD ? dsq - dB : -(dB + dsq)) * rden;
        const float dhx = fmaf(dt, r.ur, fmaf(t, d.ur, d.x)), dhz = fmaf(dt, r.uz, fmaf(t, d.uz, d.z));
        const float dnx = sg * (c * dhx), dnz = sg * (c * dhz);
        const float dcosi = -fmaf(d.ur, nx, fmaf(r.ur, dnx, fmaf(d.uz, nz, r.uz * dnz)));
        const float dsk = (eta2 * cosi * dcosi) * rev_rcp(sk);
        const float dg = fmaf(eta, dcosi, -dsk);
        d = RevRay{dhx, dhz, fmaf(eta, d.ur, fmaf(dg, nx, g * dnx)), fmaf(eta, d.uz, fmaf(dg, nz, g * dnz))};
    }
    r = RevRay{hx, hz, fmaf(eta, r.ur, g * nx), fmaf(eta, r.uz, g * nz)};
    return true;
}

ZOIC_HD int rev_uniform(int j)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(j);   // wave-uniform: the table entry is a scalar load
#else
    return j;
#endif
}

// Where an interface's eta comes from: the d-line table (RevDLine), or the indices of its two media at the point's own wavelength
// (RevSpectral, backward_spectral.hpp).  at_stop() starts a pass at the stop; then eta_front(j, S) is called for j = stop-1 ... 0, or
// eta_rear(j, S) for j = stop ... count-1.
struct RevDLine {
    ZOIC_HD void at_stop() {}
    ZOIC_HD float eta_front(int, const RevSurface &S) { return S.etaF; }
    ZOIC_HD float eta_rear(int, const RevSurface &S) { return S.etaR; }
};

// G(s): the ray leaving the stop's centre towards the front at sin(angle) = s, traced through the front group; G = the signed
// distance of Q = (rQ, zq) (zq relative to the front vertex) from the line of its exit ray, dG its derivative, scale = the larger
// component of Q - P (P the exit point).  False if the ray does not get out, or leaves away from Q.
template <class Medium>
ZOIC_HD bool rev_front(const ReverseTable &T, Medium &M, float rQ, float zq, float s, float &G, float &dG, float &scale)
{
    const float uz = rev_sqrt(fmaf(-s, s, 1.0f));
    RevRay r{0.0f, 0.0f, s, uz};
    RevRay d{0.0f, 0.0f, 1.0f, -s * rev_rcp(uz)};
    bool clipped = false;
    M.at_stop();
    for (int jj = T.stop - 1; jj >= 0; --jj) {
        const int j = rev_uniform(jj);
        if (!rev_interface<true, true>(T.surf[j], M, j, -T.surf[j + 1].dz, r, d, clipped)) return false;
    }
    const float a = rQ - r.x, b = zq - r.z;   // Q - P
    if (!(fmaf(r.ur, a, r.uz * b) > 0.0f)) return false;
    G = fmaf(r.ur, b, -(r.uz * a));
    dG = fmaf(d.ur, b, fmaf(-d.uz, a, fmaf(r.uz, d.x, -(r.ur * d.z))));
    scale = fmaxf(fabsf(a), fabsf(b));
    return true;
}

// the projection of one point: returns the flag word, writes sx, sy
template <class Medium = RevDLine>
ZOIC_HD uint32_t project_point(const ReverseTable &T, float px, float py, float pz, float &sx, float &sy, Medium M = Medium())
{
    sx = 0.0f; sy = 0.0f;
    if (T.model != 0 && T.model != 1) return kRevModelNone << kRevReasonShift;
    if (T.model == 1 && !T.domain) return kRevOutsideDomain << kRevReasonShift;
    if (!(fabsf(px) <= 3.4028235e38f && fabsf(py) <= 3.4028235e38f && fabsf(pz) <= 3.4028235e38f)) return kRevNonFinite << kRevReasonShift;
    if (T.model == 0) {   // THINLENS
        if (!(pz < 0.0f)) return kRevBehind << kRevReasonShift;
        if (px == 0.0f && py == 0.0f) return kRevProjected;
        const float inv = rev_rcp(-pz * T.tanFov);
        const float x = px * inv, y = py * inv;
        if (!(fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f)) return kRevNoRoot << kRevReasonShift;
        sx = x + 0.0f; sy = y + 0.0f;   // (+0 for a zero)
        return kRevProjected;
    }
    // RAYTRACED, trace frame: Q = -Po; meridional coordinates (rQ, zq) with the unit azimuth (ca, sa), zq relative to the front vertex
    const float qx = -px, qy = -py;
    const float zq = -pz - T.zFront;
    const float mq = fmaxf(fabsf(qx), fabsf(qy));
    float rQ = 0.0f, ca = 0.0f, sa = 0.0f;
    if (mq > 0.0f) {
        const float im = rev_rcp(mq);
        const float ax = qx * im, ay = qy * im;
        const float l = rev_sqrt(fmaf(ax, ax, ay * ay));
        rQ = mq * l;
        const float il = rev_rcp(l);
        ca = ax * il; sa = ay * il;
    }
    // behind or inside the lens: not strictly in front of the front element's cap at min(rQ, its housing radius)
    {
        const RevSurface &S0 = T.surf[0];
        const float h2 = fminf(rQ * rQ, S0.housing2);
        const float c = S0.curv;
        const float e = fmaxf(fmaf(-c * c, h2, 1.0f), 0.0f);
        const float cap = -(c * h2) * rev_rcp(1.0f + rev_sqrt(e));
        if (!(zq > 0.0f && zq > cap)) return kRevBehind << kRevReasonShift;
    }
    if (rQ == 0.0f) return kRevProjected;   // the axis is the chief ray of the centre
    // Search on s = sin(the angle at the stop).  The axis (s = 0) always gets out and has G < 0: it is one end of the bracket.  First
    // guess: the paraxial chief ray, aimed at the entrance pupil's centre.
    float s = 0.0f;
    {
        const float g = rQ * rev_rcp(zq + (T.zFront - T.zPupil)) * T.pupilSlope;
        if (g == g) s = g / (1.0f + fabsf(g));   // (a slope to a sine below 1, exact to first order)
    }
    float sNeg = 0.0f, sPos = 0.0f, sGood = 0.0f, G = 0.0f, dG = 0.0f, scale = 0.0f;
    bool havePos = false, done = false;
    for (int it = 0; it < kRevMaxIter; ++it) {
        if (!rev_front(T, M, rQ, zq, s, G, dG, scale)) {
            s = 0.5f * (s + sGood);   // no ray out there: back towards the last height that had one (the axis at first)
            continue;
        }
        sGood = s;
        if (G < 0.0f) sNeg = s; else { sPos = s; havePos = true; }
        float sn = s - G * rev_rcp(dG);
        const float lo = fminf(sNeg, sPos), hi = fmaxf(sNeg, sPos);
        const bool inside = havePos ? (sn > lo && sn < hi) : fabsf(sn) < 1.0f;
        if (fabsf(G) <= kRevTol * fmaxf(scale, T.frontRadius)) {   // converged: the last Newton step is taken without a check
            if (inside) s = sn;
            done = true;
            break;
        }
        if (!inside) sn = havePos ? 0.5f * (lo + hi) : 0.5f * (s + (sn > 0.0f ? 1.0f : -1.0f));   // bisection; towards +-1 without a bracket
        if (sn == s || (havePos && (sn == lo || sn == hi))) { done = true; break; }   // the step is below an ulp of s
        s = sn;
    }
    if (!done) return kRevNoRoot << kRevReasonShift;
    // the back group: from the stop's centre towards the rear (the stop's own refraction first), then the sensor plane
    RevRay r{0.0f, 0.0f, -s, -rev_sqrt(fmaf(-s, s, 1.0f))}, dummy{0.0f, 0.0f, 0.0f, 0.0f};
    bool clipped = false;
    M.at_stop();
    for (int jj = T.stop; jj < T.count; ++jj) {
        const int j = rev_uniform(jj);
        if (!rev_interface<false, false>(T.surf[j], M, j, jj == T.stop ? 0.0f : T.surf[j].dz, r, dummy, clipped)) return kRevNoRoot << kRevReasonShift;
    }
    // clipped in front of the stop? (the front group once more along the final ray, no tangent)
    {
        RevRay f{0.0f, 0.0f, s, rev_sqrt(fmaf(-s, s, 1.0f))};
        M.at_stop();
        for (int jj = T.stop - 1; jj >= 0; --jj) {
            const int j = rev_uniform(jj);
            if (!rev_interface<false, true>(T.surf[j], M, j, -T.surf[j + 1].dz, f, dummy, clipped)) return kRevNoRoot << kRevReasonShift;
        }
    }
    const float t = (T.sensorZ - r.z) * rev_rcp(r.uz);
    const float xs = fmaf(t, r.ur, r.x);
    const float ox = xs * ca, oy = xs * sa;   // the sensor point
    const float x = ox * T.invHalfSensor, yy = oy * T.invHalfSensor;
    if (!(fabsf(x) <= 3.4028235e38f && fabsf(yy) <= 3.4028235e38f)) return kRevNoRoot << kRevReasonShift;
    sx = x + 0.0f; sy = yy + 0.0f;
    uint32_t flags = kRevProjected | (clipped ? kRevClipped : 0u);
    if (T.useLUT) {   // the forward ray's own lookup distance (kolb_pool_body.hpp setup_ray, STRICT): |sqrt(o.x^2 + o.y^2)| of o = s halfSensor
        const float fx = sx * T.halfSensor, fy = sy * T.halfSensor;
        const float dist = fabsf(rev_sqrt(fx * fx + fy * fy));
        if (!(dist * 8.0f <= static_cast<float>(T.lutSize - 1))) flags |= kRevPastLut;
    }
    return flags;
}

// Host: the table of a camera from its LensView (backward_tables.hpp: the lens rows in trace order, rear first, after
// LensSystem::prepare), or a thin lens / NONE table.  The paraxial entrance pupil is traced in f64: the image of the stop's centre
// through the front group, n' u' = n u + y (n' - n) / R (the centre of curvature lies at vertex - R).
inline void fill_reverse_table(ReverseTable &T, const LensView &L)
{
    T = ReverseTable{};
    T.model = L.model;
    T.tanFov = L.tanFov;
    if (L.model != 1) return;
    if (!L.rows_valid()) { T.model = 2; return; }
    const int count = L.count, apertureElement = L.apertureElement;
    const float *radius = L.radius, *ior = L.ior;
    T.domain = L.domain ? 1 : 0;
    T.count = count;
    T.stop = count - 1 - apertureElement;
    T.useLUT = L.useLUT ? 1 : 0;
    T.lutSize = L.lutSize;
    T.halfSensor = L.sensorWidth * 0.5f;
    T.invHalfSensor = 1.0f / T.halfSensor;
    float vtx[kMaxSurfaces];
    backward_vertices(count, L.thickness, vtx);
    // paraxial entrance pupil: a ray from the stop's centre towards the front
    const double u0 = 0.1;
    double y = 0.0, u = u0, z = vtx[apertureElement];
    for (int i = apertureElement + 1; i < count; ++i) {
        y += u * (static_cast<double>(vtx[i]) - z);
        z = vtx[i];
        const double n = ior[i], n2 = (i + 1 < count) ? ior[i + 1] : 1.0;
        u = (n * u + y * (n2 - n) / static_cast<double>(radius[i])) / n2;
    }
    double zp = (apertureElement + 1 < count) ? z - y / u : z;
    double k = u0 / u;
    if (!std::isfinite(zp) || !std::isfinite(k) || std::fabs(zp - vtx[count - 1]) > 1.0e6) { zp = vtx[apertureElement]; k = 0.0; }   // (afocal front group: no guess)
    T.zFront = vtx[count - 1];
    T.zPupil = static_cast<float>(zp);
    T.pupilSlope = static_cast<float>(k);
    T.sensorZ = static_cast<float>(static_cast<double>(L.originShift) - static_cast<double>(vtx[0]));
    for (int j = 0; j < count; ++j) {
        const int i = count - 1 - j;
        RevSurface &S = T.surf[j];
        S.dz = (j == 0) ? 0.0f : static_cast<float>(static_cast<double>(vtx[i + 1]) - static_cast<double>(vtx[i]));
        S.curv = (i == apertureElement) ? 0.0f : static_cast<float>(1.0 / static_cast<double>(radius[i]));
        const float front = (i + 1 < count) ? ior[i + 1] : 1.0f;
        S.etaF = ior[i] / front;
        S.etaR = front / ior[i];
        S.housing2 = backward_housing2(L, i);
    }
    T.frontRadius = std::sqrt(T.surf[0].housing2);
}

// the same from flat arguments (backward_tables.hpp lens_view_of_rows)
inline void fill_reverse_table(ReverseTable &T, int model, float tanFov, int count, const float *radius, const float *thickness,
                               const float *ior, const float *aperture, int apertureElement, float userApertureRadius, float originShift,
                               float sensorWidth, bool useLUT, int lutSize, bool domain)
{
    LensView L = lens_view_of_rows(model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius);
    L.originShift = originShift; L.sensorWidth = sensorWidth; L.useLUT = useLUT; L.lutSize = lutSize; L.domain = domain;
    fill_reverse_table(T, L);
}

// ---- launcher (reverse.hip) --------------------------------------------------------------------------------------------
// d_points = n x 3 floats (packed), d_screen = n x 2 floats, d_flags = n uint32 or NULL.  Asynchronous on `stream`.
int launch_project_points(const ReverseTable &T, const float *d_points, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream);

}  // namespace zoic

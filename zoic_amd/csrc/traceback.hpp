// traceback.hpp -- trace-back (zoic_trace_back_rays_device, zoic_trace_back_ray): the screen sample Ps = (sx, sy) on which a given
// camera ray lands after travelling BACK through the lens, and whether it gets there at all.  The reference has the pieces
// (raySphereIntersection(.., reverse = true, ..), zoic.cpp:973-995) but never uses them; camera_reverse_ray returns false.  The
// reverse projection (reverse.hpp) answers for the CHIEF ray of a point; this answers for one particular ray -- what a light tracer
// or a splatter needs for depth of field, where the rays around the chief ray make the bokeh, the cat's eye and the aperture clip.
//
// Definition.
//   Input      a camera ray as the forward calls write it: zoic_ray origin and dir in the frame of the records (after the flips of
//              zoic.cpp:1845 / 1960-1961), dir pointing away from the camera into the scene (dir.z < 0).  origin is any point of the
//              ray's line in front of the lens; dir need not be unit length.  Weight and flags of the record are not read.
//   RAYTRACED  trace frame: the ray starts at q = -origin and travels along b = +dir (the forward ray reversed, b.z < 0).  The
//              interfaces are visited front -> rear (trace-order index lensCount-1 ... 0).  At each one:
//                - the sphere's vertex-side intersection, the point the forward trace takes (zoic.cpp:986; for a ray going -z the
//                  reference's `reverse` root tca - thc sign); a miss ends the ray (kTbMiss);
//                - x^2 + y^2 against Surface::housing2, the forward kernels' own limit (the stop's holds min(housing, user aperture)^2)
//                  (kTbClipped);
//                - refraction from the front-side medium into the rear-side one, eta = ior[i+1] / ior[i] (1.0 in front of the front
//                  element); total internal reflection when eta^2 (1 - cos^2) > 1 (kTbTir).
//              The stop is the reference's sphere (curvature 1 / R, |R| ~ 1e4 cm), not a plane: its sag h^2 / 2R times the ray's
//              slope would shift the clip decision by up to ~1e-4 relative at a wide stop, and the vertex form below makes the
//              sphere as cheap and as well conditioned as the plane.
//              After interface 0 the ray must still go -z; it meets the plane z = originShift at (x, y);
//              Ps = (x, y) / (sensorWidth 0.5) -- sy scaled by the WIDTH too (zoic.cpp:1853-1854).  Nothing is clipped at the sensor.
//   THINLENS   with useDof: the lens point P = the line's crossing of z = 0, accepted iff |P| <= apertureRadius and, with
//              opticalVignettingDistance > 0, the test of zoic.cpp:1297-1305 on this ray passes (kTbClipped otherwise); F = the
//              line's crossing of z = -focalDistance; Ps = F.xy / (focalDistance tan_fov).
//              (The forward path does not quite keep to that disk: the reference's disk sampler, zoic.cpp:686-704, turns its sample
//              with the parabola fast_cos / fast_sin, whose cos^2 + sin^2 reaches 2 x 0.7078125^2 = 1.001997 at phi = +-pi/4, so
//              about 0.06 % of a frame's forward records have their lens point up to 0.1 % outside apertureRadius.  Those records
//              are refused here: the aperture is the nominal disk, not the sampler's overshoot.)
//              Without DOF (a pinhole passes no generic ray) and for lensModel NONE: kTbModel (the reverse projection answers there).
//   Cameras outside the geometric FAST domain (as for reverse.hpp): kTbOutsideDomain.
//   Flags      bit 0  traced back: the ray reaches the sensor unclipped, Ps is written
//              bit 2  the sensor radius lies beyond the exit-pupil LUT's last key (as kRevPastLut)
//              bits 8-11, when bit 0 is clear: kTbAway (dir.z >= 0, or the start point is not in front of the front element's cap),
//                         kTbMiss, kTbClipped, kTbTir, kTbNonFinite (a NaN / inf coordinate, dir = 0, Ps overflows), kTbModel,
//                         kTbOutsideDomain
//              bits 16-21, for kTbMiss / kTbClipped / kTbTir: the trace-order index of the interface where the ray ended
//              A ray that is not traced back gets Ps = (+0, +0).
//
// Arithmetic.  As reverse.hpp: f32 with explicit fmaf and contraction off, correctly rounded square roots and reciprocals (device:
// exact_math.hpp; host: sqrtf and 1.0f / x), the same in every precision mode, so the host build and the kernel give the same bits.
// 3-D (skew rays).  z is kept RELATIVE to the current vertex and every sphere is taken in its vertex form c (x^2+y^2+z^2) + 2z = 0:
// no cancellation of two |R|-sized terms, at the stop's |R| ~ 1e4 either.  The start point is first moved along the line to the
// front vertex plane with the direction AS GIVEN (one fmaf per coordinate: the product is exact, so the moved point lies on
// the caller's line to an ulp of its own size) -- a start point 1e4 cm away costs no precision; only then is dir normalised.
//
// Host- and device-callable (ZOIC_HD): tests/test_traceback_cpu.py drives the host build against an f64 restatement.
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

constexpr uint32_t kTbTraced = 1u, kTbPastLut = 4u;
constexpr uint32_t kTbReasonShift = 8u, kTbInterfaceShift = 16u;
enum : uint32_t { kTbAway = 1u, kTbMiss = 2u, kTbClipped = 3u, kTbTir = 4u, kTbNonFinite = 5u, kTbModel = 6u, kTbOutsideDomain = 7u,
                  kTbWavelength = 8u };   // (kTbWavelength: the spectral calls only, backward_spectral.hpp)
constexpr float kTbMaxFloat = 3.4028235e38f;
// the start point may lie behind the front element's cap by this share of the front housing radius: a forward record's origin lies ON
// that surface, to the rounding of the forward trace
constexpr float kTbCapSlack = 6.103515625e-05f;   // 2^-14

#if defined(__HIP_DEVICE_COMPILE__)
ZOIC_HD float tb_sqrt(float x) { return sqrt_rn(x); }
ZOIC_HD float tb_rcp(float x) { return rcp_rn(x); }
#else
ZOIC_HD float tb_sqrt(float x) { return sqrtf(x); }
ZOIC_HD float tb_rcp(float x) { return 1.0f / x; }
#endif

// One interface, front-to-rear order (entry j is trace-order index count-1-j).
struct alignas(16) TbSurface {   // one 16-byte entry: one scalar load per interface
    float dz;         // vertex of the previous interface (the one in front) minus this vertex: the z step between their frames; 0 for entry 0
    float curv;       // 1 / radius (the stop: 1 / its |R| ~ 1e4 sphere)
    float eta;        // towards the rear: ior of the front-side medium / ior of the rear-side medium
    float housing2;   // clip limit on x^2 + y^2 (== Surface::housing2)
};

// Filled by the host at zoic_camera_update; a kernel argument by value (wave-uniform: scalar loads).
struct TraceBackTable {
    int32_t model;        // ZOIC_THINLENS 0, ZOIC_RAYTRACED 1, ZOIC_LENS_NONE 2
    int32_t domain;       // RAYTRACED: 1 inside the geometric domain, 0 outside (every ray reported kTbOutsideDomain)
    int32_t count;        // interfaces
    int32_t useLUT;       // kolbSamplingLUT: flag bit 2 is set against lutSize
    int32_t lutSize;
    int32_t useDof;       // THINLENS
    int32_t ovOn;         // THINLENS: opticalVignettingDistance > 0
    float halfSensor;     // sensorWidth * 0.5 (zoic.cpp:1853-1854)
    float invHalfSensor;  // 1 / halfSensor
    float sensorZ;        // the sensor plane relative to the rear vertex: originShift - vertex(rear)
    float zFront;         // the front vertex, trace frame
    float capSlack;       // kTbCapSlack x the front housing radius
    float aperture2;      // THINLENS: apertureRadius^2
    float ovDistance;     // THINLENS: opticalVignettingDistance
    float ovLimit;        // THINLENS: apertureRadius * opticalVignettingRadius (zoic.cpp:1303)
    float focalDistance;  // THINLENS: |focalDistance| (zoic.cpp:1798)
    float invFocalTan;    // THINLENS: 1 / (|focalDistance| tan_fov)
    float pad[3];
    TbSurface surf[kMaxSurfaces];
};

// Kernels with an instance per lens model (pupil_bounds.hip, splat.hip): the host picks the instance of the camera's model, and the
// kernel tells the compiler which one it is, so that each instance carries only its own model's trace (the table fields of the other
// one are not held in scalar registers across its loops).  kModelNoLens: every model that traces no ray (lensModel NONE).  Same
// operations, same bits.
constexpr int kModelThin = 0, kModelKolb = 1, kModelNoLens = 2;

template <class Kernel>
inline Kernel model_instance(const TraceBackTable &T, Kernel thin, Kernel kolb, Kernel noLens)
{
    return T.model == kModelThin ? thin : T.model == kModelKolb ? kolb : noLens;
}

#if defined(__HIPCC__)
template <int kModel>
__device__ __forceinline__ void assume_model(const TraceBackTable &T)
{
    if (kModel == kModelNoLens) __builtin_assume(T.model != kModelThin && T.model != kModelKolb);
    else __builtin_assume(T.model == kModel);
}
#endif

ZOIC_HD int tb_uniform(int j)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(j);   // wave-uniform: the table entry is a scalar load
#else
    return j;
#endif
}

ZOIC_HD uint32_t tb_end(uint32_t reason, int interface) { return (reason << kTbReasonShift) | (static_cast<uint32_t>(interface) << kTbInterfaceShift); }

ZOIC_HD bool tb_finite(float a, float b, float c) { return fabsf(a) <= kTbMaxFloat && fabsf(b) <= kTbMaxFloat && fabsf(c) <= kTbMaxFloat; }

// Where an interface's eta comes from: the d-line table (TbDLine), or the indices of its two media at the ray's own wavelength
// (TbSpectral, backward_spectral.hpp).  eta(j, S) is called once per interface, front to rear.
struct TbDLine {
    ZOIC_HD float eta(int, const TbSurface &S) { return S.eta; }
};

// What rides along with the trace: tb_trace calls these five members at fixed points of the one primal sequence, so whatever they
// compute, Ps and flags are the same operations on the same operands.  TbNoTangents carries nothing (trace_back_ray);
// TbFourTangents (traceback_jacobian.hpp) carries the four tangents of the Jacobian.
struct TbNoTangents {
    ZOIC_HD void line(float, float, float) {}                          // (dx, dy, 1 / dz): the direction has passed its guards
    ZOIC_HD void thin(const TraceBackTable &, float, float) {}         // (T, s, sf): THINLENS, Ps is written
    ZOIC_HD void seed(float, float, float) {}                          // (u): at the front vertex plane, before the first interface
    ZOIC_HD void interface(float, float, float, float, float, float, float, float, float, float, float, float) {}
                                                                       // (c, t, n, cosi, eta, sqrt(k2), g, u): u BEFORE the refraction
    ZOIC_HD void sensor(const TraceBackTable &, float, float, float, float, float, float, float) {}
                                                                       // (T, t, 1 / u.z, u.x, u.y, s, im, il): Ps and flags are settled
};

// the trace-back of one ray with G riding along: returns the flag word, writes sx, sy
template <class Medium, class Tangents>
ZOIC_HD uint32_t tb_trace(const TraceBackTable &T, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy, Medium &M,
                          Tangents &G)
{
    sx = 0.0f; sy = 0.0f;
    if (T.model != 0 && T.model != 1) return kTbModel << kTbReasonShift;
    if (T.model == 0 && !T.useDof) return kTbModel << kTbReasonShift;
    if (T.model == 1 && !T.domain) return kTbOutsideDomain << kTbReasonShift;
    if (!tb_finite(ox, oy, oz) || !tb_finite(dx, dy, dz)) return kTbNonFinite << kTbReasonShift;
    const float m = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
    if (!(m > 0.0f)) return kTbNonFinite << kTbReasonShift;
    if (!(dz < 0.0f)) return kTbAway << kTbReasonShift;
    // the unit direction (scaled by its largest component first: no overflow, no underflow of the squares)
    const float im = tb_rcp(m);
    const float ax = dx * im, ay = dy * im, az = dz * im;
    const float il = tb_rcp(tb_sqrt(fmaf(ax, ax, fmaf(ay, ay, az * az))));
    float ux = ax * il, uy = ay * il, uz = az * il;
    const float idz = tb_rcp(dz);
    if (!tb_finite(im, il, idz)) return kTbNonFinite << kTbReasonShift;
    G.line(dx, dy, idz);

    if (T.model == 0) {   // THINLENS (record frame: the lens in z = 0, the scene at z < 0)
        if (!(oz <= 0.0f)) return kTbAway << kTbReasonShift;
        const float s = -oz * idz;   // to the lens plane, along the direction as given
        const float px = fmaf(s, dx, ox), py = fmaf(s, dy, oy);
        if (!tb_finite(s, px, py)) return kTbNonFinite << kTbReasonShift;
        if (!(fmaf(px, px, py * py) <= T.aperture2)) return tb_end(kTbClipped, 0);
        if (T.ovOn) {   // empericalOpticalVignetting, zoic.cpp:1297-1305: |dir * distance - origin| (x, y) < apertureRadius * radius
            const float vx = fmaf(ux, T.ovDistance, -px), vy = fmaf(uy, T.ovDistance, -py);
            if (!(tb_sqrt(fmaf(vx, vx, vy * vy)) < T.ovLimit)) return tb_end(kTbClipped, 0);
        }
        const float sf = -T.focalDistance * idz;   // from the lens plane to z = -focalDistance
        const float fx = fmaf(sf, dx, px), fy = fmaf(sf, dy, py);
        const float x = fx * T.invFocalTan, y = fy * T.invFocalTan;
        if (!(fabsf(x) <= kTbMaxFloat && fabsf(y) <= kTbMaxFloat)) return kTbNonFinite << kTbReasonShift;
        sx = x + 0.0f; sy = y + 0.0f;   // (+0 for a zero)
        G.thin(T, s, sf);
        return kTbTraced;
    }

    // RAYTRACED, trace frame: q = -origin, b = +dir.  In front of the front element's cap at min(|q.xy|, its housing radius)?
    {
        const TbSurface &S0 = T.surf[0];
        const float zq = -oz - T.zFront;
        const float h2 = fminf(fmaf(ox, ox, oy * oy), S0.housing2);
        const float c = S0.curv;
        const float e = fmaxf(fmaf(-c * c, h2, 1.0f), 0.0f);
        const float cap = -(c * h2) * tb_rcp(1.0f + tb_sqrt(e));
        if (!(zq >= cap - T.capSlack)) return kTbAway << kTbReasonShift;
    }
    // along the line to the front vertex plane (z = zFront of the trace frame; computeLensCenters puts the front vertex at 0 to the
    // rounding of its f32 sums), with the direction as given; then z relative to the front vertex
    const float s = (oz + T.zFront) * idz;
    float x = fmaf(s, dx, -ox), y = fmaf(s, dy, -oy), z = fmaf(s, dz, -oz) - T.zFront;
    if (!tb_finite(x, y, z) || !(fabsf(s) <= kTbMaxFloat)) return kTbNonFinite << kTbReasonShift;
    G.seed(ux, uy, uz);
    for (int jj = 0; jj < T.count; ++jj) {
        const int j = tb_uniform(jj);
        const TbSurface S = T.surf[j];   // the whole entry at once
        const int iface = T.count - 1 - jj;
        const float c = S.curv;
        const float zr = z + S.dz;
        // the vertex-side root of c |p + t u|^2 + 2 (p + t u).z = 0, i.e. c t^2 + 2 B t + F = 0, for a ray going -z: of t = (-B +- sq) / c
        // the one whose hit has the larger sgn(R) z (zoic.cpp:986), which for u.z < 0 is t = (-B - sq) / c whatever the sign of c.
        // While B <= 0 (always near the axis, where B ~ u.z) that is written -F / (B - sq): no cancellation, and a plane (c = 0)
        // needs no case of its own.  B > 0 only occurs far out on a strongly curved surface (c (p . u) outweighs u.z): then
        // -(B + sq) adds two numbers of one sign and the division by c is safe (c = 0 would give B = u.z < 0).
        const float F = fmaf(c, fmaf(x, x, fmaf(y, y, zr * zr)), zr + zr);
        const float B = fmaf(c, fmaf(x, ux, fmaf(y, uy, zr * uz)), uz);
        const float disc = fmaf(-c, F, B * B);
        if (!(disc >= 0.0f)) return tb_end(kTbMiss, iface);
        const float sq = tb_sqrt(disc);
        const bool near = B <= 0.0f;
        const float rden = tb_rcp(near ? B - sq : c);
        const float t = (near ? -F : -(B + sq)) * rden;
        const float hx = fmaf(t, ux, x), hy = fmaf(t, uy, y), hz = fmaf(t, uz, zr);
        if (!(fmaf(hx, hx, hy * hy) <= S.housing2)) return tb_end(hx == hx && hy == hy ? kTbClipped : kTbMiss, iface);
        // the unit normal on the sphere, (c x, c y, 1 + c z): it points towards +z, against the ray
        const float nx = c * hx, ny = c * hy, nz = fmaf(c, hz, 1.0f);
        const float cosi = -fmaf(ux, nx, fmaf(uy, ny, uz * nz));
        const float eta = M.eta(j, S), eta2 = eta * eta;
        const float k2 = fmaf(eta2, cosi * cosi, 1.0f - eta2);
        if (!(k2 >= 0.0f)) return tb_end(kTbTir, iface);
        const float sk = tb_sqrt(k2);
        const float g = fmaf(eta, cosi, -sk);
        G.interface(c, t, nx, ny, nz, cosi, eta, sk, g, ux, uy, uz);   // with the ray's direction BEFORE the refraction
        ux = fmaf(eta, ux, g * nx); uy = fmaf(eta, uy, g * ny); uz = fmaf(eta, uz, g * nz);
        x = hx; y = hy; z = hz;
    }
    if (!(uz < 0.0f)) return tb_end(kTbMiss, 0);   // turned round at the rear element: no sensor point
    const float iuz = tb_rcp(uz);
    const float t = (T.sensorZ - z) * iuz;
    const float px = fmaf(t, ux, x) * T.invHalfSensor, py = fmaf(t, uy, y) * T.invHalfSensor;
    if (!(fabsf(px) <= kTbMaxFloat && fabsf(py) <= kTbMaxFloat)) return kTbNonFinite << kTbReasonShift;
    sx = px + 0.0f; sy = py + 0.0f;
    uint32_t flags = kTbTraced;
    if (T.useLUT) {   // the forward ray's own lookup distance, as project_point takes it
        const float fx = sx * T.halfSensor, fy = sy * T.halfSensor;
        const float dist = fabsf(tb_sqrt(fx * fx + fy * fy));
        if (!(dist * 8.0f <= static_cast<float>(T.lutSize - 1))) flags |= kTbPastLut;
    }
    G.sensor(T, t, iuz, ux, uy, s, im, il);
    return flags;
}

template <class Medium = TbDLine>
ZOIC_HD uint32_t trace_back_ray(const TraceBackTable &T, float ox, float oy, float oz, float dx, float dy, float dz, float &sx, float &sy,
                                Medium M = Medium())
{
    TbNoTangents G;
    return tb_trace(T, ox, oy, oz, dx, dy, dz, sx, sy, M, G);
}

// Host: the table of a camera from its LensView (backward_tables.hpp: the lens rows in trace order, rear first, after
// LensSystem::prepare; the stop's row carries the reference's |R| ~ 1e4 sphere), or a thin lens / NONE table.
inline void fill_traceback_table(TraceBackTable &T, const LensView &L)
{
    T = TraceBackTable{};
    T.model = L.model;
    if (L.model == 0) {
        T.useDof = L.useDof ? 1 : 0;
        T.ovOn = L.ovDistance > 0.0f ? 1 : 0;
        T.aperture2 = L.apertureRadius * L.apertureRadius;
        T.ovDistance = L.ovDistance;
        T.ovLimit = L.apertureRadius * L.ovRadius;
        T.focalDistance = std::fabs(L.focalDistance);
        T.invFocalTan = 1.0f / (T.focalDistance * L.tanFov);
        return;
    }
    if (L.model != 1) return;
    if (!L.rows_valid()) { T.model = 2; return; }
    const int count = L.count;
    T.domain = L.domain ? 1 : 0;
    T.count = count;
    T.useLUT = L.useLUT ? 1 : 0;
    T.lutSize = L.lutSize;
    T.halfSensor = L.sensorWidth * 0.5f;
    T.invHalfSensor = 1.0f / T.halfSensor;
    float vtx[kMaxSurfaces];
    backward_vertices(count, L.thickness, vtx);
    T.zFront = vtx[count - 1];
    T.sensorZ = static_cast<float>(static_cast<double>(L.originShift) - static_cast<double>(vtx[0]));
    for (int j = 0; j < count; ++j) {
        const int i = count - 1 - j;
        TbSurface &S = T.surf[j];
        S.dz = (j == 0) ? 0.0f : static_cast<float>(static_cast<double>(vtx[i + 1]) - static_cast<double>(vtx[i]));
        S.curv = static_cast<float>(1.0 / static_cast<double>(L.radius[i]));
        const float front = (i + 1 < count) ? L.ior[i + 1] : 1.0f;
        S.eta = front / L.ior[i];
        S.housing2 = backward_housing2(L, i);
    }
    T.capSlack = kTbCapSlack * std::sqrt(T.surf[0].housing2);
}

// the same from flat arguments (backward_tables.hpp lens_view_of_rows)
inline void fill_traceback_table(TraceBackTable &T, int model, float tanFov, int count, const float *radius, const float *thickness,
                                 const float *ior, const float *aperture, int apertureElement, float userApertureRadius, float originShift,
                                 float sensorWidth, bool useLUT, int lutSize, bool domain, float apertureRadius, float focalDistance,
                                 bool useDof, float ovDistance, float ovRadius)
{
    LensView L = lens_view_of_rows(model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius);
    L.originShift = originShift; L.sensorWidth = sensorWidth; L.useLUT = useLUT; L.lutSize = lutSize; L.domain = domain;
    L.apertureRadius = apertureRadius; L.focalDistance = focalDistance; L.useDof = useDof; L.ovDistance = ovDistance; L.ovRadius = ovRadius;
    fill_traceback_table(T, L);
}

// ---- launcher (traceback.hip) ------------------------------------------------------------------------------------------
// d_rays = n 32-byte zoic_ray records (16-byte aligned), d_screen = n x 2 floats (8-byte aligned), d_flags = n uint32 or NULL.
// Asynchronous on `stream`.
int launch_trace_back(const TraceBackTable &T, const void *d_rays, uint64_t n, float *d_screen, uint32_t *d_flags, void *stream);

}  // namespace zoic

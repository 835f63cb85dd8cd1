// backward_tables.hpp -- what fill_reverse_table (reverse.hpp), fill_traceback_table (traceback.hpp) and fill_ghost_table (ghost.hpp)
// take from a camera: the LensView, and the two terms they all derive from its rows (trace order, rear first).  Host only, plain
// C++: the tests' host drivers compile the headers without HIP.
#pragma once
#include <cmath>

#include "tables.hpp"

namespace zoic {

// What the table fillers read of a camera.  A value-initialised view is lensModel NONE; each model sets only its own group of fields
// (a filler reads none of another model's).
struct LensView {
    int model = 2;                    // 0 THINLENS, 1 RAYTRACED, 2 NONE
    float tanFov = 0.0f;
    // RAYTRACED: the lens rows in trace order after LensSystem::prepare (cm).  The library's view has count <= kMaxSurfaces (the parser
    // refuses longer lenses); a flat-argument caller's count is kept as given, and the fillers turn one outside 1 ... kMaxSurfaces,
    // or a stop outside the rows, into a NONE table
    int count = 0;
    float radius[kMaxSurfaces] = {}, thickness[kMaxSurfaces] = {}, ior[kMaxSurfaces] = {}, aperture[kMaxSurfaces] = {};
    int apertureElement = -1;         // the stop's row
    float userApertureRadius = 0.0f, originShift = 0.0f, sensorWidth = 0.0f;
    bool useLUT = false;              // the forward kernels sample through the exit-pupil LUT ...
    int lutSize = 0;                  // ... of this many entries (0: the lens has none)
    bool domain = false;              // the lens is inside the FAST modes' domain
    // THINLENS
    float apertureRadius = 0.0f, focalDistance = 0.0f;
    bool useDof = false;
    float ovDistance = 0.0f, ovRadius = 0.0f;   // optical vignetting

    // a RAYTRACED view a table can be made of
    bool rows_valid() const { return count >= 1 && count <= kMaxSurfaces && apertureElement >= 0 && apertureElement < count; }
};

// A view's model and rows from flat arrays (a NULL array is not read): what a caller with plain C arguments holds.  The fillers'
// flat-argument forms below their LensView forms go through it; the library itself builds the view field by field (capi.cpp).
inline LensView lens_view_of_rows(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior,
                                  const float *aperture, int apertureElement, float userApertureRadius)
{
    LensView L;
    L.model = model; L.tanFov = tanFov; L.count = count; L.apertureElement = apertureElement; L.userApertureRadius = userApertureRadius;
    for (int i = 0; i < count && i < kMaxSurfaces; ++i) {
        if (radius) L.radius[i] = radius[i];
        if (thickness) L.thickness[i] = thickness[i];
        if (ior) L.ior[i] = ior[i];
        if (aperture) L.aperture[i] = aperture[i];
    }
    return L;
}

// computeLensCenters, zoic.cpp:963-969: the vertex of every interface, the f32 running sum of the thicknesses
inline void backward_vertices(int count, const float *thickness, float *vtx)
{
    float summed = 0.0f;
    for (int i = 0; i < count; ++i) {
        summed = (i == 0) ? thickness[0] : summed + thickness[i];
        vtx[i] = summed;
    }
}

// Surface::housing2 (lens_system.cpp fill_surfaces), the forward kernels' own clip limit: the largest f32 <= (aperture / 2)^2, at
// the stop also <= userApertureRadius^2; of row i
inline float backward_housing2(const LensView &L, int i)
{
    const double half = static_cast<double>(L.aperture[i]) * 0.5, lim = half * half;
    float h = static_cast<float>(lim);
    if (static_cast<double>(h) > lim) h = std::nextafterf(h, -INFINITY);
    const float userAperture2 = L.userApertureRadius * L.userApertureRadius;
    if (i == L.apertureElement && userAperture2 < h) h = userAperture2;
    return h;
}

}  // namespace zoic

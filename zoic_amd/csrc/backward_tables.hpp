// backward_tables.hpp -- what fill_reverse_table (reverse.hpp) and fill_traceback_table (traceback.hpp) both take from the lens rows
// (trace order, rear first).  Host only, plain C++: the tests' host drivers compile the two headers without HIP.
#pragma once
#include <cmath>

namespace zoic {

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
// the stop also <= userApertureRadius^2
inline float backward_housing2(float aperture, bool atStop, float userApertureRadius)
{
    const double half = static_cast<double>(aperture) * 0.5, lim = half * half;
    float h = static_cast<float>(lim);
    if (static_cast<double>(h) > lim) h = std::nextafterf(h, -INFINITY);
    const float userAperture2 = userApertureRadius * userApertureRadius;
    if (atStop && userAperture2 < h) h = userAperture2;
    return h;
}

}  // namespace zoic

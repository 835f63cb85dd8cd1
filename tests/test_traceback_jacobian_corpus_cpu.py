"""The trace-back Jacobian on the pinned corpus of machine-made lenses (machine_lens_corpus.py: 5 ... 14 interfaces, the stop at trace
index 0, near-hemispherical rear elements, a V column, a camera outside the geometric domain) and at scene distances, without a GPU:
the host build of csrc/traceback_jacobian.hpp (zoic_trace_back_ray_jacobian and its spectral form on tables-only cameras) against f64
central differences (traceback_jacobian_ref.py).

Every lens.  On the corpus ray set machine_lens_corpus.ray_set (a stride of the live forward records, the rejection families,
random lines, the non-finite rays) and 1 024 far rays (jr.far_rays: live records moved 30 ... 1e4 cm out along the ray, every other
one with dir scaled by 1e3 or 1e-3), about 7 000 rays a lens: Ps and flags are zoic_trace_back_ray's bits, J is twelve +0.0 where
bit 0 is clear, and J is finite and nonzero on every traced ray the f64 trace puts off TraceBack.edge; the same with
bs.mixed_wavelengths, where a rejected wavelength is reported first and 587.5618 nm gives the d-line's bits, J included.  At the
d-line the library traces back all of the far rays but a handful; petzval-5 refuses every ray kTbOutsideDomain, Ps and J all zero bits.

The six accuracy lenses.  test_traceback_jacobian_cpu.accuracy's procedure (jr.measure), unchanged: every 16th live record (petzval-2:
every 8th), dir normalised in f64, the rays the f64 trace takes back off the edge set with all reference and yardstick neighbours
traced, nine yardstick steps 2^-6 ... 2^-14, at most 3 % of the picked rays left out at the yardstick's step, by the library's and by
the f64 trace's decisions alike.  Errors are |(J - Jref) S|_F / |Jref S|_F.
  near   the start point one front housing radius s_o out, S = diag(s_o, s_o, s_o, 1, 1, 1), Jref from the plain f64 trace at the steps
         1e-6 s (used) and 1e-5 s; d-line, and spectral with 16 wavelengths over [400, 700] nm spread across the rays;
  far    the start point k = 30, 200 (= |focalDistance|), 3 000 and 1e4 cm out along the ray, cast to f32; S = diag(s_o, s_o, s_o, s_o / k,
         s_o / k, s_o / k) for J, Jref and the yardstick alike; Jref through jr.near_trace (every neighbour moved along its own line to
         the plane one s_o in front of the front vertex before the f64 trace: the module's docstring says why) at the steps 1e-5 s
         (used) and 1e-4 s -- mori-6 and fisheye-5, whose h^2 term is the largest, at 1e-6 s (used) and 1e-5 s.
The requirement, the project's own: J's median <= the yardstick's / 4 and J's p99 <= the yardstick's, at the yardstick's eligible step
and at its best step of any.  Reference soundness, asserted first: near, Jref's two steps agree to 1e-7 (fisheye-5: to 3.8e-7, twice
the 1.9e-7 its d-line reference alone gives; its spectral reference gives 3.2e-7); far, to a tenth of J's median on that lens and
distance -- every one of the 24 cells gets there (the worst: mori-6 at 1e4 cm, 0.087 of J's median), so none is left unasserted.
Null vectors near:
|J_o dir| <= 2.3e-9 and |J_d dir| <= 4.3e-8 of |J S|_F (bound: the p99 error of the same rays).  Measured (host build):

    lens, start              rays   J median / p99        yardstick h, median / p99      best median of any h   Jref's two steps: max (steps)
    triplet-4, near           1559  1.09e-07 / 3.01e-07   2^-9  1.29e-05 / 3.14e-05    1.02e-05 (2^-8)     1.85e-10 (1e-5, 1e-6)
    triplet-4 spectral, near  1559  1.24e-07 / 3.86e-07   2^-9  1.30e-05 / 3.05e-05    1.01e-05 (2^-8)     2.39e-10 (1e-5, 1e-6)
    triplet-4, 30 cm          1541  1.92e-06 / 5.95e-06   2^-7  1.89e-04 / 4.35e-04    9.60e-05 (2^-6)     1.61e-09 (1e-4, 1e-5)
    triplet-4, 200 cm         1543  4.00e-06 / 2.07e-05   2^-7  3.99e-04 / 8.25e-04    2.03e-04 (2^-6)     3.31e-09 (1e-4, 1e-5)
    triplet-4, 3000 cm        1543  3.12e-06 / 1.56e-05   2^-7  3.23e-04 / 6.50e-04    1.66e-04 (2^-6)     1.01e-08 (1e-4, 1e-5)
    triplet-4, 10000 cm       1543  3.16e-06 / 1.48e-05   2^-7  3.24e-04 / 6.33e-04    1.64e-04 (2^-6)     4.53e-08 (1e-4, 1e-5)
    fisheye-5, near           2542  5.34e-06 / 2.04e-05   2^-13 3.72e-04 / 1.48e-03    1.89e-04 (2^-12)    1.88e-07 (1e-5, 1e-6)
    fisheye-5 spectral, near  2522  4.64e-06 / 2.79e-05   2^-14 8.37e-04 / 4.80e-03    2.14e-04 (2^-12)    3.19e-07 (1e-5, 1e-6)
    fisheye-5, 30 cm          2556  6.69e-06 / 2.71e-05   2^-13 5.38e-04 / 2.49e-03    1.84e-04 (2^-11)    1.38e-07 (1e-5, 1e-6)
    fisheye-5, 200 cm         2536  8.14e-06 / 3.66e-05   2^-12 3.96e-04 / 2.03e-03    2.23e-04 (2^-11)    1.17e-07 (1e-5, 1e-6)
    fisheye-5, 3000 cm        2538  8.42e-06 / 3.68e-05   2^-12 4.29e-04 / 2.16e-03    2.31e-04 (2^-11)    1.16e-07 (1e-5, 1e-6)
    fisheye-5, 10000 cm       2538  8.30e-06 / 3.78e-05   2^-12 4.28e-04 / 2.33e-03    2.32e-04 (2^-11)    1.13e-07 (1e-5, 1e-6)
    mori-6, near              1995  5.51e-07 / 1.81e-06   2^-10 5.96e-05 / 1.29e-04    3.52e-05 (2^-9)     1.02e-09 (1e-5, 1e-6)
    mori-6 spectral, near     1990  4.95e-07 / 1.68e-06   2^-10 5.85e-05 / 1.25e-04    3.56e-05 (2^-9)     9.14e-10 (1e-5, 1e-6)
    mori-6, 30 cm             1991  8.08e-06 / 4.57e-05   2^-8  5.99e-04 / 1.16e-03    5.03e-04 (2^-7)     2.15e-08 (1e-5, 1e-6)
    mori-6, 200 cm            1992  1.23e-05 / 2.10e-04   2^-8  9.45e-04 / 4.41e-03    7.06e-04 (2^-7)     1.00e-07 (1e-5, 1e-6)
    mori-6, 3000 cm           1992  1.28e-05 / 2.99e-04   2^-8  1.02e-03 / 8.15e-03    7.75e-04 (2^-7)     2.96e-07 (1e-5, 1e-6)
    mori-6, 10000 cm          1993  1.30e-05 / 3.13e-04   2^-8  1.05e-03 / 8.52e-03    7.74e-04 (2^-7)     1.13e-06 (1e-5, 1e-6)
    double-3, near            2519  1.95e-07 / 6.02e-07   2^-8  1.54e-05 / 3.36e-05    1.54e-05 (2^-8)     4.55e-10 (1e-5, 1e-6)
    double-3 spectral, near   2532  2.18e-07 / 6.68e-07   2^-8  1.56e-05 / 3.47e-05    1.56e-05 (2^-8)     4.69e-10 (1e-5, 1e-6)
    double-3, 30 cm           2525  2.91e-06 / 1.00e-05   2^-7  1.84e-04 / 4.01e-04    1.05e-04 (2^-6)     1.33e-08 (1e-4, 1e-5)
    double-3, 200 cm          2528  1.47e-05 / 5.24e-05   2^-7  8.98e-04 / 2.32e-03    4.96e-04 (2^-6)     6.59e-08 (1e-4, 1e-5)
    double-3, 3000 cm         2529  1.12e-05 / 4.43e-05   2^-7  6.60e-04 / 2.20e-03    3.68e-04 (2^-6)     6.22e-08 (1e-4, 1e-5)
    double-3, 10000 cm        2529  1.10e-05 / 3.99e-05   2^-7  6.54e-04 / 2.20e-03    3.62e-04 (2^-6)     6.46e-08 (1e-4, 1e-5)
    tessar-5, near            1393  1.50e-07 / 4.02e-07   2^-9  1.63e-05 / 3.60e-05    7.51e-06 (2^-7)     2.50e-10 (1e-5, 1e-6)
    tessar-5 spectral, near   1391  1.36e-07 / 3.92e-07   2^-9  1.63e-05 / 3.73e-05    7.51e-06 (2^-7)     2.50e-10 (1e-5, 1e-6)
    tessar-5, 30 cm           1385  2.22e-06 / 7.54e-06   2^-7  2.89e-04 / 6.31e-04    1.46e-04 (2^-6)     2.37e-09 (1e-4, 1e-5)
    tessar-5, 200 cm          1385  1.52e-05 / 5.75e-05   2^-7  2.10e-03 / 4.43e-03    1.07e-03 (2^-6)     1.91e-08 (1e-4, 1e-5)
    tessar-5, 3000 cm         1385  1.43e-05 / 5.44e-05   2^-7  1.90e-03 / 5.71e-03    9.58e-04 (2^-6)     2.40e-08 (1e-4, 1e-5)
    tessar-5, 10000 cm        1385  1.42e-05 / 5.47e-05   2^-7  1.82e-03 / 5.76e-03    9.22e-04 (2^-6)     5.38e-08 (1e-4, 1e-5)
    petzval-2, near           1997  1.19e-07 / 3.02e-07   2^-11 4.85e-05 / 1.04e-04    1.31e-05 (2^-9)     2.84e-10 (1e-5, 1e-6)
    petzval-2 spectral, near  2016  1.33e-07 / 3.57e-07   2^-11 4.85e-05 / 1.06e-04    1.31e-05 (2^-9)     2.92e-10 (1e-5, 1e-6)
    petzval-2, 30 cm          2017  1.01e-06 / 3.50e-06   2^-8  1.90e-04 / 4.14e-04    5.02e-05 (2^-6)     1.10e-09 (1e-4, 1e-5)
    petzval-2, 200 cm         2006  3.71e-06 / 1.30e-05   2^-7  3.44e-04 / 7.00e-04    1.77e-04 (2^-6)     3.34e-09 (1e-4, 1e-5)
    petzval-2, 3000 cm        2006  2.72e-06 / 8.98e-06   2^-7  2.56e-04 / 5.29e-04    1.33e-04 (2^-6)     3.65e-09 (1e-4, 1e-5)
    petzval-2, 10000 cm       2005  2.73e-06 / 9.66e-06   2^-7  2.54e-04 / 5.18e-04    1.31e-04 (2^-6)     1.49e-08 (1e-4, 1e-5)

J's error in the distance-scaled metric is flat from 200 cm to 1e4 cm on every lens: the start-step composition J_d = s g + ... costs
nothing as s grows.  It is above the near figure (1.5 times on fisheye-5, up to 100 times on tessar-5) because the f32 start point
itself is coarser there (an ulp of 1e4 cm is 1e-3 cm): the yardstick, which reads the same inputs, stays 50 ... 130 times worse than J.

What these bounds see, tried once on a host build with one line of TbFourTangents broken: the s of J[3] / J[9] times 1 + 2^-12 fails
16 of the 24 far cells (mori-6 and tessar-5 pass: their yardstick is the coarsest), fisheye-5 near and three solid-angle tests; the
transfer's u dt dropped from dh.z at the stop (eta = 1), and d.z dropped from the sensor step, fail 30 ... 36 accuracy tests and
five or six solid-angle tests each.  The same breaks also fail three to eight of test_traceback_jacobian_cpu's accuracy tests: near
the lens s g is a tenth or more of J_d, not a negligible part.  A factor 1 + 2^-16 on the same s passes everything, there and here:
the yardstick, a quarter of which is the bound, is no finer than 4e-5 at any distance.

The three lenses held to the bitwise comparison (mori-4, rear-9, rear-12; the corpus's policy: grazing rear surfaces make an f32
bound a statement about conditioning) get the same figures near and at 3 000 cm, printed and recorded here, not bounded; J is finite
and nonzero on the kept rays.  The yardstick's step is its best of any with >= 512 rays kept:

    lens, start         rays   J median / p99        yardstick h, median / p99      left out    Jref's two steps: max
    mori-4, near        1130  2.51e-07 / 8.09e-07   2^-9  2.02e-05 / 3.87e-05     2.08 %     3.35e-10
    mori-4, 3000 cm     1116  9.99e-06 / 1.31e-04   2^-7  5.22e-04 / 4.01e-03     3.29 %     9.09e-07
    rear-9, near        1466  2.22e-06 / 1.08e-05   2^-11 3.20e-04 / 8.14e-04     2.07 %     5.94e-07
    rear-9, 3000 cm     1429  1.70e-06 / 1.10e-05   2^-8  1.69e-04 / 1.38e-03     4.54 %     1.78e-06
    rear-12, near       2380  1.55e-06 / 8.92e-06   2^-10 2.25e-04 / 4.94e-04     2.26 %     8.48e-08
    rear-12, 3000 cm    2363  1.52e-06 / 1.14e-05   2^-8  1.46e-04 / 3.91e-04     2.96 %     3.02e-07

The solid-angle measure dPs/domega = det(J_d |d| [e1 e2]) (zoic_amd.solid_angle_measure) of the library's J against the reference's on
the kept rays, the yardstick's beside it.  Asserted: the sign on every ray, and a median relative error within the yardstick's.
Recorded only: p99 and max.  Between 30 cm and 3 000 cm dPs/domega goes through zero on some rays (the start point passes the plane
the lens is focused on), and the relative error of a determinant near its zero is conditioning, not accuracy: the worst below is 0.54
(mori-6 at 200 cm) where the yardstick's is 3.9.  A splatter that divides by the measure must guard that zero itself.

    lens, start            dPs/domega (reference)        J: median / p99 / max               yardstick: median / p99 / max
    triplet-4, near          -12.05 ... -11.1       1.47e-07 / 5.70e-07 / 7.60e-07    5.75e-06 / 2.76e-05 / 4.61e-05
    triplet-4, 30 cm         -9.002 ... 0.5348      2.85e-06 / 2.53e-05 / 6.01e-04    9.91e-05 / 2.29e-03 / 3.20e-01
    triplet-4, 200 cm        -186.1 ... 0.8013      1.43e-05 / 1.40e-03 / 1.99e-02    4.01e-04 / 2.19e-02 / 1.42e+00
    triplet-4, 3000 cm   -6.684e+04 ... -1213       5.74e-06 / 3.28e-05 / 6.67e-05    1.76e-04 / 8.44e-04 / 1.28e-03
    triplet-4, 10000 cm   -7.58e+05 ... -1.542e+04  5.75e-06 / 3.17e-05 / 4.39e-05    1.75e-04 / 8.15e-04 / 1.54e-03
    fisheye-5, near          -76.94 ... -8.924      9.97e-06 / 4.34e-05 / 7.63e-05    1.74e-04 / 1.70e-03 / 3.32e-03
    fisheye-5, 30 cm         -152.6 ... -3.855      1.23e-05 / 6.24e-05 / 2.43e-04    2.75e-04 / 4.99e-03 / 2.56e-02
    fisheye-5, 200 cm         -2509 ... 268.6       1.64e-05 / 1.87e-04 / 1.59e-01    2.51e-04 / 1.26e-02 / 1.83e+00
    fisheye-5, 3000 cm    -4.51e+05 ... 6.234e+04   1.78e-05 / 3.48e-04 / 7.70e-03    2.66e-04 / 1.68e-02 / 8.29e-01
    fisheye-5, 10000 cm  -4.952e+06 ... 6.902e+05   1.76e-05 / 3.77e-04 / 4.48e-03    2.85e-04 / 1.65e-02 / 1.33e-01
    mori-6, near             -14.23 ... -10.66      9.79e-07 / 3.48e-06 / 5.78e-06    2.43e-05 / 1.21e-04 / 1.97e-04
    mori-6, 30 cm            -164.8 ... -7.439      1.33e-05 / 6.65e-05 / 9.99e-05    2.81e-04 / 1.09e-03 / 1.83e-03
    mori-6, 200 cm            -3974 ... 0.0392      2.77e-05 / 5.09e-04 / 5.40e-01    5.60e-04 / 4.87e-03 / 3.93e+00
    mori-6, 3000 cm      -7.884e+05 ... 864.6       3.46e-05 / 1.88e-03 / 1.39e-01    6.87e-04 / 3.36e-02 / 1.04e+00
    mori-6, 10000 cm     -8.706e+06 ... 1.046e+04   3.48e-05 / 2.09e-03 / 3.79e-02    6.77e-04 / 3.18e-02 / 9.58e-01
    double-3, near           -12.66 ... -11.06      2.75e-07 / 1.08e-06 / 1.58e-06    7.30e-06 / 3.07e-05 / 4.40e-05
    double-3, 30 cm          -11.96 ... -6.773      3.69e-06 / 1.46e-05 / 2.24e-05    7.35e-05 / 3.57e-04 / 6.01e-04
    double-3, 200 cm         -3.601 ... 1.42        1.52e-04 / 7.06e-03 / 2.42e-01    3.31e-03 / 2.13e-01 / 5.66e+00
    double-3, 3000 cm         -5060 ... 1255        2.08e-05 / 2.86e-04 / 2.62e-02    3.97e-04 / 1.27e-02 / 1.81e+00
    double-3, 10000 cm   -6.006e+04 ... 1.366e+04   2.00e-05 / 1.90e-04 / 6.24e-03    3.98e-04 / 8.77e-03 / 2.66e-01
    tessar-5, near           -12.56 ... -11.46      2.49e-07 / 7.90e-07 / 8.78e-07    6.19e-06 / 3.04e-05 / 4.99e-05
    tessar-5, 30 cm          -12.33 ... -8.348      2.65e-06 / 1.05e-05 / 1.45e-05    1.14e-04 / 5.51e-04 / 8.18e-04
    tessar-5, 200 cm         -8.399 ... 0.02058     7.67e-05 / 4.65e-03 / 2.78e-02    2.59e-03 / 8.42e-02 / 2.37e+00
    tessar-5, 3000 cm         -2256 ... 873.3       3.21e-05 / 8.29e-04 / 1.43e-02    1.71e-03 / 1.06e-01 / 1.86e+00
    tessar-5, 10000 cm   -2.764e+04 ... 9713        3.12e-05 / 9.79e-04 / 8.46e-03    1.44e-03 / 9.96e-02 / 8.23e-01
    petzval-2, near          -11.01 ... -10.32      1.53e-07 / 5.77e-07 / 8.31e-07    1.95e-05 / 8.76e-05 / 1.38e-04
    petzval-2, 30 cm         -7.977 ... -5.633      1.31e-06 / 5.35e-06 / 8.69e-06    8.03e-05 / 3.80e-04 / 5.79e-04
    petzval-2, 200 cm        -7.014 ... -0.005375   1.67e-05 / 1.97e-04 / 1.02e-03    5.13e-04 / 2.86e-03 / 7.22e-03
    petzval-2, 3000 cm        -7304 ... -2292       4.92e-06 / 1.83e-05 / 2.98e-05    1.53e-04 / 6.35e-04 / 9.78e-04
    petzval-2, 10000 cm  -8.556e+04 ... -2.801e+04  4.86e-06 / 1.93e-05 / 2.77e-05    1.42e-04 / 6.72e-04 / 9.64e-04
"""
import numpy as np
import pytest

from zoic_amd import solid_angle_measure

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import traceback_cases as tc
import traceback_jacobian_ref as jr
from device_cases import bits as _bits
from traceback_ref import OUTSIDE_DOMAIN

F32 = np.float32
NEAR = 0.0                                  # the key of the near case: one housing radius out
DISTANCES = (30.0, 200.0, 3000.0, 1e4)      # cm out along the ray (200 = |focalDistance| of the corpus camera)
BITWISE_FAR = 3000.0
# the reference's two steps.  Near: test_traceback_jacobian_cpu's.  Far: the dir steps are h s_o / k on a unit vector, so the pair is
# ten times larger; mori-6, whose h^2 term is the largest of the corpus, keeps the smaller pair.
NEAR_STEPS = (1e-6, 1e-5)
FAR_STEPS = {name: (1e-5, 1e-4) for name in mc.NAMES}
FAR_STEPS["mori-6"] = FAR_STEPS["fisheye-5"] = (1e-6, 1e-5)
# reference soundness near: 1e-7 as test_traceback_jacobian_cpu; where the reference alone does not reach it, twice what it gives
NEAR_SOUND = {name: 1e-7 for name in mc.ACCURACY}
NEAR_SOUND["fisheye-5"] = 2 * 1.9e-7


class _Lens:
    """one corpus lens: its tables-only camera, the f64 trace and the live oracle records of the frame (dir normalised in f64)"""

    def __init__(self, oracle_lib, name):
        self.name = name
        self.cam, self.p = mc.camera(name)
        self.info = self.cam.info()
        self.T = bs.SpectralTraceBack(self.info, self.p, self.cam.dispersion())
        self.s = jr.scales(self.info, self.p)
        _, o, d, w = mc.oracle_records(oracle_lib, name)
        self.o, self.d = np.ascontiguousarray(o[w > 0], F32), jr.unit_f32(d[w > 0])
        self.plane = jr.front_plane(self.T, self.s)
        self.rays = mc.ray_set(oracle_lib, self.cam, name)[0]


_LENSES, _ACC = {}, {}


def _lens(oracle_lib, name):
    if name not in _LENSES:
        _LENSES[name] = _Lens(oracle_lib, name)
    return _LENSES[name]


def bit_rays(L):
    """the corpus ray set (machine_lens_corpus.ray_set) and the far set: (origin, dir)"""
    fo, fd = jr.far_rays(L.o, L.d)
    return (np.ascontiguousarray(np.concatenate([L.rays[:, 0:3], fo]), F32), np.ascontiguousarray(np.concatenate([L.rays[:, 3:6], fd]), F32))


def accuracy(oracle_lib, name, k=NEAR, spectral=False):
    """test_traceback_jacobian_cpu.accuracy's procedure on a corpus lens.  k = NEAR: the start point one housing radius out, the plain
    f64 trace, the scales jr.scales.  Otherwise the start point k cm out (cast to f32), the f64 trace through jr.near_trace and the
    scales jr.far_scales(s, k).  Cached."""
    key = (name, k, spectral)
    if key in _ACC:
        return _ACC[key]
    L = _lens(oracle_lib, name)
    stride = 16
    while stride > 1 and len(L.o[::stride]) * (1.0 - jr.LEFT_OUT_CAP) < jr.MIN_RAYS:
        stride //= 2
    d = L.d[::stride]
    out = L.s[0] if k == NEAR else k
    o = (L.o[::stride].astype(np.float64) + out * d.astype(np.float64)).astype(F32)
    lam = np.linspace(400.0, 700.0, 16).astype(F32)[np.arange(len(o)) % 16] if spectral else None   # spread over the rays

    def trace(O, D):
        return L.T.trace_at(O, D, np.tile(lam, len(O) // len(lam))) if spectral else L.T.trace(O, D)

    if k == NEAR:
        s, steps = L.s, NEAR_STEPS
    else:
        trace, s, steps = jr.near_trace(trace, L.plane), jr.far_scales(L.s, k), FAR_STEPS[name]
    tag = "%s%s %s" % (name, " spectral" if spectral else "", "near" if k == NEAR else "%g cm" % k)
    A = jr.measure(L.cam, trace, L.T.edge, o, d, lam, s, ref_steps=steps, tag=tag)
    _ACC[key] = dict(A, p=L.p, T=L.T, stride=stride, tag=tag, steps=steps)
    return _ACC[key]


def _soundness(A, kept):
    return float(jr.rel_error(A["Jref5"][kept], A["Jref"][kept], A["s"]).max())


def _null_vectors(A, kept):
    J, d = A["J"][kept].astype(np.float64), A["d"][kept].astype(np.float64)
    scale = np.sqrt(((J * A["s"][None, None, :]) ** 2).sum((1, 2)))
    no = np.linalg.norm(np.einsum("nij,nj->ni", J[:, :, :3], d), axis=1) / scale
    nd = np.linalg.norm(np.einsum("nij,nj->ni", J[:, :, 3:] * A["s"][3], d), axis=1) / scale
    return float(no.max()), float(nd.max())


# ---- 1. bits, zeros and finiteness on every lens -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_ps_flags_and_untraced_j_on_every_corpus_lens(oracle_lib, name):
    """Ps and flags are zoic_trace_back_ray's bits, J is twelve +0.0 where nothing is traced, and nonzero and finite on every traced
    ray the f64 trace puts off the edge set -- at the d-line and with bs.mixed_wavelengths (the f64 edge set at the wavelengths
    rounded to whole nanometres); at 587.5618 nm the spectral call gives the d-line's bits, J included."""
    L = _lens(oracle_lib, name)
    O, D = bit_rays(L)
    near = jr.near_trace(L.T.trace, L.plane)
    ps, fl, J = jr.host_jacobian(L.cam, O, D)
    ps0, fl0 = jr.host_trace(L.cam, O, D)
    assert np.array_equal(_bits(ps), _bits(ps0)) and np.array_equal(fl, fl0)
    traced = (fl & 1) == 1
    assert not _bits(J[~traced]).any()
    ps1, fl1, J1 = jr.host_jacobian(L.cam, O, D, jr.LAMBDA_D)
    assert np.array_equal(_bits(ps1), _bits(ps)) and np.array_equal(fl1, fl) and np.array_equal(_bits(J1), _bits(J))
    lam = bs.mixed_wavelengths(len(O))
    bad = ~bs.valid(lam)
    ps2, fl2, J2 = jr.host_jacobian(L.cam, O, D, lam)
    ps3, fl3 = jr.host_trace(L.cam, O, D, lam)
    assert np.array_equal(_bits(ps2), _bits(ps3)) and np.array_equal(fl2, fl3)
    traced2 = (fl2 & 1) == 1
    assert not _bits(J2[~traced2]).any()
    assert bad.sum() > len(O) // 5 and (fl2[bad] == bs.TB_WAVELENGTH << 8).all()      # a rejected wavelength comes first
    at_d = lam == F32(bs.LAMBDA_D)
    assert at_d.sum() > len(O) // 20 and np.array_equal(_bits(J2[at_d]), _bits(J[at_d])) and np.array_equal(_bits(ps2[at_d]), _bits(ps[at_d]))
    if name == mc.OUTSIDE:
        assert (fl == OUTSIDE_DOMAIN << 8).all() and (fl2[~bad] == OUTSIDE_DOMAIN << 8).all()
        assert not _bits(ps).any() and not _bits(J).any() and not _bits(ps2).any() and not _bits(J2).any()
        return
    n_far = len(O) - len(L.rays)
    for tag, f, t, j, ref in (("d-line", fl, traced, J, near(O, D)),
                              ("mixed wavelengths", fl2, traced2, J2, jr.near_trace(lambda o, d: L.T.trace_at(o, d, np.round(lam)), L.plane)(O, D))):
        good = t & ref["traced"] & ~L.T.edge(ref)
        print("%s %s: %d rays, %d traced (%d of the %d far ones), %d of them off the f64 edge; refused for the reasons %s" % (
            name, tag, len(O), t.sum(), t[-n_far:].sum(), n_far, good.sum(), sorted(set(tc.reason(f[~t]).tolist()))))
        assert good.sum() > 0.9 * t.sum() and t[-n_far:].sum() > (0.5 if j is J else 0.3) * n_far
        assert np.isfinite(j[good]).all() and (np.abs(j[good]).max((1, 2)) > 0).all()
        assert len(set(tc.reason(f[~t]).tolist())) >= 4


# ---- 2. accuracy near and far on the six accuracy lenses ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_near_reference_is_sound(oracle_lib, name):
    """the reference at the steps 1e-6 s and 1e-5 s, on the kept rays one housing radius out"""
    for spectral in (False, True):
        A = accuracy(oracle_lib, name, NEAR, spectral)
        e = _soundness(A, jr.best(A)["kept"])
        print("%s: Jref(1e-5) against Jref(1e-6): max %.3g (bound %.3g)" % (A["tag"], e, NEAR_SOUND[name]))
        assert e <= NEAR_SOUND[name], e


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_near_accuracy_against_the_finite_difference_yardstick(oracle_lib, name):
    A = accuracy(oracle_lib, name)
    jr.check_accuracy(A, A["tag"])


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_near_spectral_accuracy_against_the_finite_difference_yardstick(oracle_lib, name):
    A = accuracy(oracle_lib, name, NEAR, True)
    jr.check_accuracy(A, A["tag"])


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_near_null_vectors(oracle_lib, name):
    """J_o . dir = 0 and J_d . dir = 0, to the p99 error of the accuracy test"""
    for spectral in (False, True):
        A = accuracy(oracle_lib, name, NEAR, spectral)
        best = jr.best(A)
        no, nd = _null_vectors(A, best["kept"])
        print("%s: |J_o d| max %.3g, |J_d d| max %.3g, p99 error %.3g" % (A["tag"], no, nd, best["j_p99"]))
        assert no <= best["j_p99"] and nd <= best["j_p99"], (no, nd, best["j_p99"])


@pytest.mark.parametrize("k", DISTANCES)
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_far_accuracy_against_the_finite_difference_yardstick(oracle_lib, name, k):
    """The start point k cm out, the reference through near_trace, every figure in the distance-scaled S.  The reference's two steps
    must agree to a tenth of J's median before J is held to the yardstick."""
    A = accuracy(oracle_lib, name, k)
    best = jr.best(A)
    e = _soundness(A, best["kept"])
    no, nd = _null_vectors(A, best["kept"])
    print("%s: Jref(%g) against Jref(%g): max %.3g = %.3g of J's median; |J_o d| max %.3g, |J_d d| max %.3g" % (
        A["tag"], A["steps"][1], A["steps"][0], e, e / best["j_med"], no, nd))
    assert e <= 0.1 * min(best["j_med"], best["y_med"] / 4.0), (e, best["j_med"], best["y_med"])
    jr.check_accuracy(A, A["tag"])


# ---- 3. the lenses held to the bitwise comparison: recorded, not bounded -----------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in mc.BITWISE if n != mc.OUTSIDE])
def test_bitwise_only_lenses_are_recorded(oracle_lib, name):
    """the corpus's policy for them: the same figures near and at 3 000 cm, printed; J finite on every candidate ray"""
    for k in (NEAR, BITWISE_FAR):
        A = accuracy(oracle_lib, name, k)
        rows = [r for r in A["rows"] if r["kept"].sum() >= jr.MIN_RAYS // 2]
        assert rows, A["tag"]
        r = min(rows, key=lambda r: r["y_med"])
        print("%s: stride %d, %d rays kept at h = 2^%d (left out %.2f %%, by the f64 trace alone %.2f %%): J median %.3g p99 %.3g; yardstick "
              "median %.3g p99 %.3g; Jref's two steps: max %.3g (not bounded)" % (
                  A["tag"], A["stride"], r["kept"].sum(), round(np.log2(r["h"])), 100 * r["left_out"], 100 * r["left_out64"], r["j_med"],
                  r["j_p99"], r["y_med"], r["y_p99"], _soundness(A, r["kept"])))
        assert np.isfinite(A["J"][r["kept"]]).all() and (np.abs(A["J"][r["kept"]]).max((1, 2)) > 0).all()


# ---- 4. the solid-angle measure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_solid_angle_measure(oracle_lib, name):
    """dPs/domega = det(J_d |d| [e1 e2]) of the library's J against the reference's, near and far, the yardstick's beside it.  Asserted:
    the sign, and a median relative error within the yardstick's.  p99 and max are recorded: close to the focus distance dPs/domega
    goes through zero and its relative error is conditioning."""
    for k in (NEAR,) + DISTANCES:
        A = accuracy(oracle_lib, name, k)
        best = jr.best(A)
        kept = best["kept"]
        d = A["d"][kept].astype(np.float64)
        want = solid_angle_measure(A["Jref"][kept], d)
        got = solid_angle_measure(A["J"][kept].astype(np.float64), d)
        yard = solid_angle_measure(best["Y"][kept], d)
        eg, ey = np.abs(got - want) / np.abs(want), np.abs(yard - want) / np.abs(want)
        print("%s: dPs/domega %.4g ... %.4g; relative error median %.3g p99 %.3g max %.3g; yardstick (h = 2^%d) median %.3g p99 %.3g max %.3g"
              % (A["tag"], want.min(), want.max(), np.median(eg), np.percentile(eg, 99), eg.max(), round(np.log2(best["h"])),
                 np.median(ey), np.percentile(ey, 99), ey.max()))
        assert (want != 0).all() and np.array_equal(np.sign(got), np.sign(want))
        assert np.median(eg) <= np.median(ey), (np.median(eg), np.median(ey))

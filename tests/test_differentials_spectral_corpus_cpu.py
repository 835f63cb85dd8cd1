"""Traced ray differentials of spectral records on the pinned corpus of machine-made lenses (machine_lens_corpus.py: 5 ... 14
interfaces, the stop at trace index 0, near-hemispherical rear elements, a five-column lens with its own V column, glasses whose
V-numbers differ in file order), without a GPU: the host build of csrc/differentials_spectral.hpp (host_drivers.differentials_spectral) against f64 central differences of the numpy restatement, started from differentials_ref.kolb_start on the oracle's d-line
records of the frame traceback_cases.frame_samples().

Inputs shared with tests/test_differentials_spectral_corpus_gpu.py: differentials_spectral_corpus.py (the frame and one wavelength
per ray, the rows that get the f64 reference, the reference itself, the conditioning rule and the figures).

Conditioning rule, the d-line fuzz's own (tests/test_differentials_fuzz_gpu.py): a ray whose f64 trace at its own wavelength meets an
interface with min |cos| below COS_MIN = 0.05 (sref.min_cos_incidence) has no reliable finite difference and is left out of the
accuracy comparison only.  The share left out may not exceed EDGE_CAP = 0.02 of a lens's live rays, and the f64 restatement must
reproduce the records within differentials_ref.restatement_holds: both are asserted on the reference alone before any output of the
library is read.  Measured on the reference alone (the oracle's d-line records, strided to at most 4 096; `passes`: the share of them
that also pass at their wavelength in f64, differentials_spectral_ref.passes with the housing apertures):

    lens       rays  passes  excluded  restatement: eo median, ed median / 99.9th   retried
    triplet-4  3738  0.9997  0.0000    3.61e-07, 1.27e-07 / 4.46e-07                240
    fisheye-5  3947  1.0000  0.0000    4.88e-07, 1.46e-07 / 4.83e-07               1190
    mori-6     3728  0.9989  0.0000    7.94e-07, 1.71e-07 / 5.04e-07                326
    double-3   3913  0.9997  0.0000    3.54e-07, 1.49e-07 / 4.75e-07               1256
    tessar-5   3816  0.9995  0.0000    3.74e-07, 1.49e-07 / 5.08e-07                969
    petzval-2  3669  0.9984  0.0000    4.28e-07, 1.12e-07 / 3.98e-07               1460
    mori-4     3915  0.9992  0.0000    7.27e-07, 1.34e-07 / 4.72e-07                  9
    rear-9     3849  1.0000  0.0000    1.12e-06, 1.96e-07 / 1.36e-06               2946
    rear-12    3930  0.9992  0.0000    1.11e-06, 1.97e-07 / 9.65e-07               2582
    petzval-5  3597  0.9825  0.0000    6.47e-07, 1.04e-07 / 4.00e-07               1688

No ray of these sets meets an interface below COS_MIN, at the d-line's tries or (tests/test_differentials_spectral_corpus_gpu.py) at
the tries the spectral forward kernel accepts: all six lenses of machine_lens_corpus.ACCURACY stay in the accuracy group.  mori-4, rear-9
and rear-12 meet both conditions on this reference too; they keep the group machine_lens_corpus gives them (BITWISE) and are held to
the identities and to the d-line kernel as the yardstick, as the backward paths hold them.

The accuracy group (ACCURACY) is what of machine_lens_corpus.ACCURACY meets both conditions; IDENTITIES_ONLY names every other lens
with its reason.  On the accuracy group, the host build against the reference (test_differentials_spectral_cpu's bounds unchanged:
screen tangents median <= 1e-5 and 99.9th percentile <= 1e-3; wavelength tangent against the sum of its interfaces' contributions and
against its own size at most 4 x the screen figures; halving the wavelength step moves the central difference by less than 4 x the
screen median).  Measured (host build, CPU only; median / 99.9th percentile; cancellation: sum |contributions| / |dD/dlambda|):

    lens       rays  excluded  screen s_med / s_tail   contributions c_med / c_tail   own size l_med / l_tail   cancellation
    triplet-4  3738  0.0000    1.65e-07 / 3.37e-06     5.04e-09 / 5.62e-08            2.56e-08 / 7.95e-08        7.9
    fisheye-5  3947  0.0000    2.17e-07 / 1.01e-06     8.34e-09 / 4.32e-08            2.55e-08 / 8.23e-08        3.3
    mori-6     3728  0.0000    6.38e-07 / 5.71e-06     3.11e-09 / 1.39e-08            2.47e-08 / 7.77e-08        7.1
    double-3   3913  0.0000    2.71e-07 / 1.48e-06     7.40e-09 / 4.38e-08            2.49e-08 / 7.69e-08        3.4
    tessar-5   3816  0.0000    2.38e-07 / 3.22e-06     9.26e-10 / 4.30e-09            2.64e-08 / 8.32e-08       20.8
    petzval-2  3669  0.0000    2.83e-07 / 1.97e-06     1.72e-09 / 7.50e-09            2.54e-08 / 7.59e-08       15.4

At 587.5618 nm every lens of the corpus, petzval-5 included, gives kolb_differentials' bits in modes 1 and 2.

A wrong index is caught: with `cauchyB[i + 1]` of kolb_wavelength_tangent read as `cauchyB[i]` in a scratch copy of the header,
test_tangents_match_finite_differences and test_wavelength_tangent_ratio_to_its_own_size fail on all of the accuracy lenses (every
one has distinct V-numbers): c_med goes from 9.3e-10 ... 8.3e-9 to 7.7e-2 (triplet-4) ... 4.3e-1 (fisheye-5), l_med from 2.5e-8 to 0.75 ... 5.2, the screen tangents unchanged.
"""
import numpy as np
import pytest

import differentials_ref as dref
import differentials_spectral_ref as sref
import machine_lens_corpus as mc
import host_drivers
from device_cases import bits_f32 as _bits
from differentials_ref import COS_MIN
from differentials_spectral_corpus import ACCURACY, IDENTITIES_ONLY, conditions, figures, frame, line, reference, reference_rows, tables
from differentials_spectral_ref import passes as _passes
from host_drivers import run_differentials_spectral as run_driver
from machine_lens_corpus import EDGE_CAP
from spectral_ref import LAMBDA_D32, WAVES

F32 = np.float32


# ---- the start rays of this file: the oracle's d-line records -------------------------------------------------------------------
_STARTS = {}


def starts(oracle_lib, name):
    """The oracle's live d-line records of the frame behind lens `name`, reference_rows of them: their start rays by
    differentials_ref.kolb_start, their wavelengths, whether each also passes at its wavelength in f64, the replay and the
    restatement of the d-line records, and the f64 reference of those that pass."""
    if name in _STARTS:
        return _STARTS[name]
    p, info, disp, hs = tables(name)
    s, st, lam = frame()
    _, o, d, w = mc.oracle_records(oracle_lib, name)
    tries = mc.oracle_tries(oracle_lib, name)
    rows = reference_rows(np.flatnonzero(w != 0), tries)
    oc = mc.oracle_camera(oracle_lib, name)
    lt = oc.lens_table()
    surf = dref.surfaces(lt)
    o0, d0 = dref.kolb_start(oc, p, s[rows], tries[rows], st[rows], oracle_lib)
    replay, eo, ed = dref.replay_and_restatement(oc, o0, d0, o[rows], d[rows])
    oc.close()
    lam = lam[rows].copy()
    ok = _passes(surf, sref.cauchy_eta(disp, lam), o0, d0, lt["elements"][:, 3])
    S = dict(surf=surf, disp=disp, hs=hs, rows=rows[ok], o0=o0[ok], d0=d0[ok], lam=lam[ok], passes=float(ok.mean()), replay=bool(replay.all()),
             restated=dref.restatement_holds(eo, ed), eo=eo[ok], ed=ed[ok], retried=int((tries[rows[ok]] > 0).sum()))
    S["ref"] = reference(surf, disp, hs, S["lam"], S["o0"], S["d0"])
    _STARTS[name] = S
    return S


@pytest.fixture(scope="module")
def driver():
    return host_drivers.differentials_spectral()


def test_per_ray_min_cos_is_the_d_line_rule():
    """sref.min_cos_incidence is differentials_ref.min_cos_incidence where eta is uniform over the rays: the hand-made rays of
    test_differentials_fuzz_gpu.test_min_cos_incidence_rule (head-on, cos i = 0.8, grazing; eta > 1: the refracted ray grazes first)
    and a two-interface lens"""
    o = np.array([[0.0, 0.0, -5.0], [6.0, 0.0, -5.0], [9.999, 0.0, -5.0], [6.6, 0.0, -5.0]])
    d = np.array([[0.0, 0.0, 1.0]] * 4)
    for etas in ([1.0 / 1.5], [1.5], [1.0 / 1.5, 1.6]):
        surf = np.array([[10.0, 100.0, 1.0, e] for e in etas], F32)
        surf[1:, 0], surf[1:, 2] = 25.0, -1.0
        a = dref.min_cos_incidence(surf, o, d)
        b = sref.min_cos_incidence(surf, np.tile(surf[:, 3].astype(np.float64), (len(o), 1)), o, d)
        assert np.array_equal(a, b)
    one = np.array([[10.0, 100.0, 1.0, 1.0 / 1.5]], F32)
    c = sref.min_cos_incidence(one, np.full((4, 1), float(one[0, 3])), o, d)
    assert abs(c[0] - 1.0) < 1e-12 and abs(c[1] - 0.8) < 1e-12 and c[2] < COS_MIN
    # an eta per ray: the same hit, a different refraction angle
    c = sref.min_cos_incidence(one, np.array([[1.0 / 1.5], [1.5]]), o[[3, 3]], d[[3, 3]])
    assert abs(c[1] - np.sqrt(1 - 0.99 ** 2)) < 1e-9 and abs(c[0] - np.sqrt(1 - 0.66 ** 2)) < 1e-9


@pytest.mark.parametrize("name", mc.NAMES)
def test_reference_only_conditions(oracle_lib, name):
    """The conditions of the accuracy comparison on the reference alone, every lens with live records: kolb_start's start rays ARE the
    tries the oracle traced (its own f32 trace from them gives the records bit for bit); on the accuracy group the f64 restatement
    reproduces the records, the conditioning rule leaves out at most EDGE_CAP of the rays that pass at their wavelength, at least 0.95
    of the d-line's records pass at their wavelength, all eight WAVES and 200 retried rays are among them; a lens of
    IDENTITIES_ONLY is printed with the same figures."""
    S = starts(oracle_lib, name)
    good, excluded, restated = conditions(S["ref"]["cos"], S["eo"], S["ed"])
    print("%-10s rows %4d  passes %.4f  excluded %.4f  restatement %s (eo %.2e, ed %.2e / %.2e)  retried %d" % (
        name, len(S["rows"]), S["passes"], excluded, restated, np.median(S["eo"]), np.median(S["ed"]), np.percentile(S["ed"], 99.9), S["retried"]))
    assert S["replay"]
    if name in ACCURACY:
        assert S["restated"] and restated
        assert excluded <= EDGE_CAP, (name, excluded)
        assert S["passes"] >= 0.95 and good.sum() >= 1000, (name, S["passes"], good.sum())
        assert np.isin(WAVES, S["lam"][good]).all() and S["retried"] >= 200
    else:
        assert name in IDENTITIES_ONLY


def test_the_accuracy_group():
    """at least four of the six, the most and the fewest interfaces among them; every lens is in exactly one group"""
    assert len(ACCURACY) >= 4 and "fisheye-5" in ACCURACY and "triplet-4" in ACCURACY
    assert sorted(ACCURACY + list(IDENTITIES_ONLY)) == sorted(mc.NAMES)
    assert {mc.BY_NAME[n].interfaces for n in ACCURACY} >= {5, 14}


_MEASURED = {}


def _measure(name, driver, oracle_lib):
    if name in _MEASURED:
        return _MEASURED[name]
    S = starts(oracle_lib, name)
    ref = S["ref"]
    # the reference-only conditions, before the library is looked at
    good, excluded, restated = conditions(ref["cos"], S["eo"], S["ed"])
    assert S["replay"] and restated and excluded <= EDGE_CAP, (name, S["replay"], restated, excluded)
    assert S["disp"]["cauchy_b"].any()
    out, chroma, prim = run_driver(driver, 2, S["surf"], S["disp"], S["hs"], S["lam"], S["o0"], S["d0"])
    out12, chroma0, _ = run_driver(driver, 1, S["surf"], S["disp"], S["hs"], S["lam"], S["o0"], S["d0"])
    assert np.array_equal(_bits(out), _bits(out12)) and not _bits(chroma0).any()   # the third tangent changes nothing else
    assert np.isfinite(out).all() and np.isfinite(chroma).all()
    ro, rd = ref["end"]
    assert np.allclose(prim[good, 0:3], -ro[good], rtol=1e-4, atol=1e-4) and np.allclose(prim[good, 3:6], -rd[good], rtol=1e-4, atol=1e-5)
    m = figures(out, chroma, ref, good)
    print(line(name, m, excluded))
    _MEASURED[name] = m
    return m


@pytest.mark.parametrize("name", ACCURACY)
def test_tangents_match_finite_differences(name, driver, oracle_lib):
    """test_differentials_spectral_cpu.test_tangents_match_finite_differences on a corpus lens, its bounds unchanged"""
    m = _measure(name, driver, oracle_lib)
    assert m["step"] < 4 * m["s_med"], m
    assert m["s_med"] <= 1e-5 and m["s_tail"] <= 1e-3, (name, m)
    assert m["c_med"] <= 4 * m["s_med"] and m["c_tail"] <= 4 * m["s_tail"], (name, m)


@pytest.mark.parametrize("name", ACCURACY)
def test_wavelength_tangent_ratio_to_its_own_size(name, driver, oracle_lib):
    """test_differentials_spectral_cpu.test_wavelength_tangent_ratio_to_its_own_size on a corpus lens, its bounds unchanged"""
    m = _measure(name, driver, oracle_lib)
    assert m["l_med"] <= 4 * m["s_med"] and m["l_tail"] <= 4 * m["s_tail"], (name, m)


@pytest.mark.parametrize("name", mc.NAMES)
def test_d_line_gives_the_d_line_tangents(name, driver, oracle_lib):
    """at lambda = 587.5618f the 12 floats and the primal are kolb_differentials', bit for bit, in modes 1 and 2 (mode 1 == mode 2),
    on every lens of the corpus (the forward call makes records behind petzval-5 too: only the backward paths refuse it)."""
    p, info, disp, hs = tables(name)
    assert disp["cauchy_b"].any()
    S = starts(oracle_lib, name)
    surf, o, d = S["surf"], S["o0"], S["d0"]
    lam = np.full(len(o), LAMBDA_D32, F32)
    ref, _, rprim = run_driver(driver, 0, surf, disp, hs, lam, o, d)
    assert len(o) >= 1000 and (_bits(ref) != 0).any()
    for mode in (1, 2):
        got, _, prim = run_driver(driver, mode, surf, disp, hs, lam, o, d)
        assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(prim), _bits(rprim))

"""Fresnel transmittance on the pinned corpus of machine-made lenses and on plates-32, the lens that fills the tables
(tests/lens_losses_corpus.py), without a GPU: the host build of csrc/transmittance.hpp (test_transmittance_cpu's driver) against the
f64 restatement (transmittance_ref.transmittance), bare and with a film wherever the media differ, and against the host build of
trace_lens_spectral_strict for where a path passes at all.

Starts: differentials_ref.kolb_start on the oracle's d-line records of the frame traceback_cases.frame_samples(), all of reference_rows
of the live ones (at most 4096: the restatement is one vectorised pass, so it runs on every row), at the wavelengths of
differentials_spectral_corpus.frame().  The records pass at the d-line; at its own wavelength a start may not.  Only starts
that pass in f64 are compared: the f64 path meets every sphere, is nowhere totally reflected (transmittance_ref) and stays within the
housings (ghost_ref.ghost's plain path).  Their share is asserted on the reference alone, before the host build is read.  Beyond a
relative margin of PASS_MARGIN on every decision of the f64 path the host build must pass the same starts; the few nearer ones that it
clips (T = 0) are left out of the error.

Measured (host build: clang++ 22, x86-64, CPU only): the share of the starts that pass in f64, the rows compared, the
largest |host build - f64| of T bare / with the film, the f64 T's median bare / with the film:

    lens       starts  pass in f64   rows    error bare / film      T median bare / film
    triplet-4  3 739   0.9997        3 738   1.39e-7 / 1.73e-7      0.762 / 0.973
    fisheye-5  3 947   0.9997        3 946   1.90e-7 / 3.38e-7      0.528 / 0.891
    mori-6     3 732   0.9989        3 728   1.78e-7 / 3.09e-7      0.470 / 0.938
    double-3   3 914   0.9985        3 908   2.24e-7 / 2.73e-7      0.592 / 0.850
    tessar-5   3 818   0.9995        3 816   2.04e-7 / 2.51e-7      0.677 / 0.863
    petzval-2  3 675   0.9984        3 669   2.36e-7 / 2.02e-7      0.741 / 0.906
    mori-4     3 918   0.9992        3 915   2.00e-7 / 2.42e-7      0.676 / 0.852
    rear-9     3 849   0.9078        3 494   1.08e-6 / 1.38e-6      0.679 / 0.922
    rear-12    3 933   0.9558        3 759   5.17e-7 / 6.72e-7      0.679 / 0.922
    petzval-5  3 661   0.9760        3 573   2.39e-7 / 3.11e-7      0.664 / 0.851
    plates-32  3 942   0.9982        3 935   1.46e-7 / 4.13e-7      0.206 / 0.696

On every lens the host build passes exactly the starts the f64 path passes: none is left out.

MEASURED_ACCURACY and MEASURED_OTHERS hold the largest error on the six lenses of machine_lens_corpus.ACCURACY and on the other five;
both are asserted with the project's 4 x for other compilers' host builds.  test_transmittance_cpu.BOUND (1.34e-6, from C2 - C5) would
not hold on rear-9, and one bound taken from rear-9 would be four times looser than the other lenses need."""
import ctypes

import numpy as np
import pytest

import ghost_ref as gref
import lens_losses_corpus as lc
import machine_lens_corpus as mc
import transmittance_ref as tref
import host_drivers
from device_cases import bits_f32 as _bits
from host_drivers import run_transmittance as run_driver

F32 = np.float32
PASS_MARGIN = 5e-3       # test_ghost_cpu._plain's: the STRICT trace's rounding at the stop's sphere decides nothing beyond it
MIN_ROWS = 2048          # starts of a lens that pass in f64
# the share of a lens's starts that must pass in f64 at their own wavelength: the near-hemispherical rear elements, mori-4 and
# petzval-5 (machine_lens_corpus.BITWISE) lose up to a tenth of the d-line's records to the wavelength, the others 2 in 1000
MIN_SHARE = {name: 0.85 if name in mc.BITWISE else 0.99 for name in lc.NAMES}
# Largest |host build - f64 restatement| of T over the runs of test_host_build_against_f64, bare and film
MEASURED_ACCURACY = 3.384e-7  # fisheye-5 with the film; the six lenses of mc.ACCURACY
MEASURED_OTHERS = 1.382e-6    # rear-9 with the film; mori-4, rear-9, rear-12, petzval-5 and plates-32


def _measured(name):
    return MEASURED_ACCURACY if name in mc.ACCURACY else MEASURED_OTHERS


@pytest.fixture(scope="module")
def driver():
    return host_drivers.transmittance()


@pytest.fixture(scope="module")
def gdriver():
    return host_drivers.ghost()


def test_the_corpus_is_the_pinned_one():
    """the texts by their crc32 and the shape of the tables; every lens has a V-number per glass, so the media on both sides of every
    interface depend on the wavelength; the film sits exactly where the media differ"""
    for name in lc.NAMES:
        assert lc.crc(name) == (lc.PLATES_CRC if name == lc.PLATES else mc.BY_NAME[name].crc), name
        T = lc.tables(name)
        assert (T["count"], T["stop"], len(T["pairs"]), T["equal"]) == lc.SHAPE[name], name
        glass = T["disp"]["ior_d"] != 1
        assert T["disp"]["cauchy_b"][glass].all() and not T["disp"]["cauchy_b"][~glass].any(), name
        coated = T["film"][0] != 0
        assert coated.sum() == T["count"] - 1 - len(T["equal"]) and not coated[T["stop"]] and not coated[list(T["equal"])].any()
    assert sorted(mc.ACCURACY + mc.BITWISE + [lc.PLATES]) == sorted(lc.NAMES)


_REFERENCE = {}


def _reference(oracle_lib, name):
    """the f64 T of every start, bare and with the film, and which starts pass in f64 -- no library output is read"""
    if name not in _REFERENCE:
        T, S = lc.tables(name), lc.starts(oracle_lib, name)
        bare, ok = tref.transmittance(T["surf"], T["disp"], S["lam"], S["o"], S["d"])
        film, ok2 = tref.transmittance(T["surf"], T["disp"], S["lam"], S["o"], S["d"], *T["film"])
        assert np.array_equal(ok, ok2)
        plain = gref.ghost(T["L"], T["disp"], S["lam"], S["o"], S["d"], -1, -1)
        passes = ok & (plain["reason"] == gref.TRACED)
        sure = plain["margin"] >= PASS_MARGIN
        # the two restatements are the same physics in two geometries, the one about the centres of the camera's table, the other about
        # vertex - R of the f32 vertex sums: the plain path's weight is the bare T as far as those f32 centres agree
        assert np.abs(plain["weight"][passes & sure] - bare[passes & sure]).max() <= 1e-6
        _REFERENCE[name] = dict(bare=bare, film=film, passes=passes, sure=sure, good=passes)
    return _REFERENCE[name]


@pytest.mark.parametrize("name", lc.NAMES)
def test_reference_alone_has_the_rows(oracle_lib, name):
    """on the reference alone: at least MIN_SHARE of the starts pass in f64 at their wavelength, at least MIN_ROWS rows; their T lies
    in (0, 1), the film's above the bare one"""
    R = _reference(oracle_lib, name)
    good = R["good"]
    print("%-10s starts %4d  pass %.4f (%d rows), with the margin %.4f" % (name, len(good), good.mean(), good.sum(), (good & R["sure"]).mean()))
    assert good.mean() >= MIN_SHARE[name] and good.sum() >= MIN_ROWS, (name, good.mean(), int(good.sum()))
    assert (R["bare"][good] > 0).all() and (R["film"][good] < 1).all() and (R["film"][good] > R["bare"][good]).all()


_MEASURED = {}


def _measure(name, coated, driver, oracle_lib):
    key = (name, coated)
    if key not in _MEASURED:
        T, S, R = lc.tables(name), lc.starts(oracle_lib, name), _reference(oracle_lib, name)
        good = R["good"]
        assert good.mean() >= MIN_SHARE[name] and good.sum() >= MIN_ROWS          # the reference first
        got = run_driver(driver, T["surf"], T["disp"], S["lam"], S["o"], S["d"], T["film"] if coated else None, T["housing2"])
        ref = R["film" if coated else "bare"]
        # a start whose f64 path passes by less than the margin may be clipped in f32 (T = 0): left out, and there are few
        assert (got[good & R["sure"]] > 0).all() and (got < 1).all()
        left_out = good & (got == 0)
        assert left_out.mean() <= 1e-3, (name, int(left_out.sum()))
        good = good & (got > 0)
        _MEASURED[key] = dict(rows=int(good.sum()), share=float(good.mean()), err=float(np.abs(got.astype(np.float64) - ref)[good].max()),
                              t_med=float(np.median(ref[good])), got=got, left_out=int(left_out.sum()))
        print("%-10s %-5s rows %4d (%.4f, %d left out)  err %.3e  T median %.3f" % (
            name, "film" if coated else "bare", _MEASURED[key]["rows"], _MEASURED[key]["share"], left_out.sum(), _MEASURED[key]["err"], _MEASURED[key]["t_med"]))
    return _MEASURED[key]


@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_host_build_against_f64(name, coated, driver, oracle_lib):
    """|host build - f64 restatement| of T from the same starts, every start that passes in f64 and in the
    host build (they pass the same starts beyond the margin): at most 4 x
    MEASURED_ACCURACY on the lenses of machine_lens_corpus.ACCURACY, 4 x MEASURED_OTHERS on the others and on plates-32; T > 0 on all
    of them.  The table is in the module docstring."""
    m = _measure(name, coated, driver, oracle_lib)
    assert m["err"] <= 4 * _measured(name), (name, m["err"])


def test_measured_bounds_are_the_measured_ones(driver, oracle_lib):
    for group, measured in (([n for n in lc.NAMES if n in mc.ACCURACY], MEASURED_ACCURACY), ([n for n in lc.NAMES if n not in mc.ACCURACY], MEASURED_OTHERS)):
        assert len(group) >= 5
        worst = max(_measure(name, coated, driver, oracle_lib)["err"] for name in group for coated in (False, True))
        assert measured / 4 <= worst <= 4 * measured, (group, worst)


@pytest.mark.parametrize("name", lc.NAMES)
def test_zero_exactly_where_the_host_path_does_not_pass(name, driver, gdriver, oracle_lib):
    """every start, bare and film: T is +0.0 exactly where the host build of trace_lens_spectral_strict (the forward kernels' trace,
    with the housings) does not pass from that start at that wavelength, and lies in (0, 1) elsewhere; the film changes no path.  Where
    the f64 path decides with the margin the host build decides the same."""
    T, S, R = lc.tables(name), lc.starts(oracle_lib, name), _reference(oracle_lib, name)
    surf, disp = T["surf"], T["disp"]
    s4 = np.ascontiguousarray(np.stack([surf[:, 0], surf[:, 1], surf[:, 2], T["housing2"]], 1), F32)
    dp = np.ascontiguousarray(np.stack([disp["ior_d"], disp["cauchy_b"]], 1), F32)
    o, d, lam = (np.ascontiguousarray(v, F32) for v in (S["o"], S["d"], S["lam"]))
    out = np.zeros((len(o), 7), F32)
    fp = ctypes.POINTER(ctypes.c_float)
    passed = gdriver.zgh_strict(len(surf), s4.ctypes.data_as(fp), dp.ctypes.data_as(fp), len(o), lam.ctypes.data_as(fp), o.ctypes.data_as(fp),
                                d.ctypes.data_as(fp), out.ctypes.data_as(fp))
    passes = out[:, 6] != 0
    assert passed == passes.sum()
    for coated in (False, True):
        got = _measure(name, coated, driver, oracle_lib)["got"]
        assert np.array_equal(got > 0, passes) and not _bits(got[~passes]).any() and (got[passes] < 1).all()
    assert np.array_equal(passes[R["sure"]], R["passes"][R["sure"]])
    if name in ("rear-9", "rear-12", "petzval-5"):
        assert (~passes).sum() >= 50, (name, int((~passes).sum()))      # the zeros are exercised

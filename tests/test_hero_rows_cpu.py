"""The rows form of a hero call (tests/hero_rows.py) on the reference alone, before tests/test_hero_rows_gpu.py relies on it: no GPU.

For every case of hero_rows.CASES, on the cached reference of the hero call (hero_cases.reference):
  1  every through companion's f64 trace from the recorded start at the companion's own wavelength comes through (sref.passes); the
     rows where it does not are left out of every comparison,
  2  and reproduces the reference's own companion record (differentials_ref.restatement_holds);
  3  at most machine_lens_corpus.EDGE_CAP of the through companions are left out;
  4  the host build of csrc/differentials_spectral.hpp (driver mode 2) from those starts meets tests/test_differentials_spectral_gpu.py's
     bounds against sref.jacobian_fd, sref.wavelength_fd and sref.wavelength_contributions;
  5  at least hero_cases.FAMILY_MIN of the compared rows belong to retried heroes;
  6  the host build of csrc/ghost.hpp from the same starts, over the pairs the device test runs, bare and coated, yields at least 1000
     traced and 1000 ended ghosts (tests/test_ghost_gpu.py's census), every lost row ending as NO_START.

Measured (through companions / of retried heroes / left out; restatement medians eo, ed; host build against f64: screen tangents
median and 99.9th percentile, wavelength tangent against its contributions median; ghosts traced / ended, bare):

    case          rows   retried  left out  eo        ed        screen tangents       contributions  ghosts
    C2             9158    557    0         3.6e-07   1.4e-07   2.42e-07 / 5.61e-06   1.06e-09       109900 / 234164
    C2-nolut       6599   6259    0         3.7e-07   1.4e-07   2.39e-07 / 5.39e-06   1.07e-09        36263 /  94809
    C3-bokeh-V50  11670   2117    0         3.8e-07   1.6e-07   2.98e-07 / 1.69e-06   5.56e-09        56800 /  74272
    triplet-4      6837    105    0         3.7e-07   1.3e-07   1.64e-07 / 3.38e-06   5.20e-09        63245 /  67827
    fisheye-5     11823   1092    0         4.8e-07   1.5e-07   2.34e-07 / 1.05e-06   8.54e-09        47138 /  83934
    mori-6         8811    114    0         7.7e-07   1.8e-07   6.35e-07 / 5.73e-06   3.13e-09        17548 / 113524
    C5-k8          4562   1613    0         5.9e-07   1.1e-07   3.36e-07 / 1.60e-06   2.60e-09         8703 / 253441

A film changes no path: the coated census is the bare one.

The one cap of the device module that the reference alone cannot show is the 0.999 of rows on which a STRICT and a FAST camera agree: it
is a statement about two device runs (FAST may end a hero at another try than STRICT only inside its guard bands), so the device module
measures and prints it per camera before it asserts."""
import numpy as np
import pytest

import differentials_ref as dref
import differentials_spectral_corpus as dsc
import ghost_ref as gref
import hero_cases as hr
import hero_rows as hw
import host_drivers
from host_drivers import run_differentials_spectral, run_ghost_records
from machine_lens_corpus import EDGE_CAP

F32 = np.float32


@pytest.mark.parametrize("case", hw.CASES)
def test_rows_form(oracle_lib, case):
    """flat() is the issue's definition, row by row; the classes partition the rows; a companion's start is its hero's"""
    R = hw.rows(oracle_lib, case)
    assert R.k == hw.CASES[case][1] and R.n == hr.N and len(R.lam_r) == R.n * R.k
    for r in (0, 1, R.k - 1, R.k, 5 * R.k + 3, R.n * R.k - 1):
        i, j = divmod(r, R.k)
        assert (R.hero[r], R.col[r]) == (i, j)
        assert np.array_equal(R.samples_r[r], R.samples[i]) and np.array_equal(R.states_r[r], R.states[i]) and R.lam_r[r] == R.lam[i, j]
        assert np.array_equal(R.words_r[r], R.words[i, j])
    assert not (R.cls == hw.REJECTED).any()                      # the reference's palette holds valid wavelengths only
    live_hero = np.repeat(R.words[:, 0, 6] != 0, R.k)
    lost = (R.cls == hw.LOST) & (R.col >= 1)
    assert ((R.words_r[lost, 7] & hr.LOST) != 0).all() and not R.words_r[lost, :7].any()
    assert (lost & live_hero).sum() >= hr.FAMILY_MIN             # lost companions of live heroes are among the rows
    assert not (R.words_r[R.through_companions, 7] & hr.LOST).any() and live_hero[R.through_companions].all()
    assert np.array_equal(R.words_r[R.through_companions, 6:8], R.words[R.hero[R.through_companions], 0, 6:8])   # the hero's weight and flags
    assert R.starts_r[R.through_companions].any(1).all()


@pytest.mark.parametrize("case", hw.CASES)
def test_reference_of_the_through_companions(oracle_lib, case):
    """items 1-5"""
    R, T, X = hw.rows(oracle_lib, case), hw.tables(case), hw.f64(oracle_lib, case)
    good = X["good"]
    assert len(X["rows"]) >= 2048
    assert X["left_out"] <= EDGE_CAP, X["left_out"]
    assert dref.restatement_holds(X["eo"][good], X["ed"][good]), (float(np.median(X["eo"][good])), float(np.median(X["ed"][good])))
    assert X["retried"] >= hr.FAMILY_MIN, X["retried"]
    out, ch, prim = run_differentials_spectral(host_drivers.differentials_spectral(), 2, T.surf, T.disp, T.hs, X["lam"], X["o0"], X["d0"])
    rec = R.words_r[X["rows"], 0:6].copy().view(F32)
    assert np.allclose(prim[good], rec[good], rtol=1e-5, atol=1e-5)
    m = dsc.figures(out, ch, X["ref"], good)
    print("%-13s rows %5d retried %5d left out %d  eo %.1e ed %.1e  %s" % (
        case, len(good), X["retried"], (~good).sum(), np.median(X["eo"][good]), np.median(X["ed"][good]), dsc.line(case, m, X["left_out"])))
    assert np.isfinite(out[good]).all() and np.isfinite(ch[good]).all()
    assert hw.spectral_bounds_hold(m), m


@pytest.mark.parametrize("case", hw.CASES)
def test_ghost_census_of_the_rows(oracle_lib, case):
    """item 6, bare and coated; lost rows end as NO_START whatever else holds for them"""
    R, T = hw.rows(oracle_lib, case), hw.tables(case)
    assert len(T.pairs) == (21 if case == hw.ALL_PAIRS else 8) and (T.pairs[:, 0] > T.pairs[:, 1]).all()
    for film in (None, T.film):
        g = run_ghost_records(host_drivers.ghost(), T.lens, T.disp, R.lam_r, R.starts_r[:, 0:3], R.starts_r[:, 3:6], T.pairs, have=R.weight != 0, film=film)
        traced, ended = hw.ghost_census(g)
        print("%-13s %s ghosts traced %d ended %d" % (case, "bare  " if film is None else "coated", traced, ended))
        assert traced >= hw.GHOST_MIN and ended >= hw.GHOST_MIN
        words = np.ascontiguousarray(g).view(np.uint32)
        dead = np.zeros(8, np.uint32)
        dead[7] = gref.flag_word(gref.NO_START)
        assert (words[R.cls == hw.LOST] == dead).all()
        assert (words[R.through_companions][..., 7] == 1).any(1).mean() > 0.5      # the companions' rows carry ghosts of their own


def test_thin_case_reference(oracle_lib):
    """group G's camera: the reference repeats the hero's record in every column, and some heroes retry (the stream matters)"""
    sp = hw.spec(hw.THIN)
    s, lam, st = hr.inputs(hr.N, 4, 11)
    words, _ = hr.hero_reference(oracle_lib, sp.params, None, s, lam, st)
    assert (words[:, 1:] == words[:, :1]).all()
    live = words[:, 0, 6] != 0
    assert live.sum() >= 1000 and (~live).sum() >= hr.FAMILY_MIN and (live & (((words[:, 0, 7] >> 1) & 31) > 0)).sum() >= hr.FAMILY_MIN

"""Ghost rays on the pinned corpus of machine-made lenses and on plates-32, the lens that fills the tables (tests/lens_losses_corpus.py),
without a GPU: the host build of csrc/ghost.hpp (test_ghost_cpu's driver) against the f64 restatement in plain sphere geometry
(ghost_ref.ghost) on every pair of ghost_pairs(), bare and coated; the plain path against the host builds of
trace_lens_spectral_strict and path_transmittance; and the cases the hand-picked cameras of test_ghost_cpu.py cannot make: interface
counts 5 ... 14 and 32, the stop at trace index 0, NO_REFLECTION on an interface that is not the stop, a leg that crosses an interface
between equal media, more than 32 pairs.

Starts: differentials_ref.kolb_start on the oracle's d-line records of the frame traceback_cases.frame_samples(), reference_rows of
the live ones (at most 4096), at the wavelengths of differentials_spectral_corpus.frame().  The f64 restatement runs on a
stride of at most 1024 of them (plates-32: 128), all pairs.  MARGIN and MAX_LEFT_OUT are test_ghost_cpu's, unchanged.

The corpus (test_the_corpus_is_the_pinned_one).  `equal`: interfaces other than the stop between equal media at the d-line.  Only two
lenses have one: they are air rows that meet where an element was dropped or an air row was doubled; a doubled glass row is perturbed
after it is copied, so its two copies differ.

    lens       interfaces  stop  pairs  equal
    triplet-4       5        2      6
    fisheye-5      14        5     55   6, 9
    mori-6         11        0     45
    double-3       12        6     55
    tessar-5       10        6     36
    petzval-2      10        4     28   0
    mori-4          9        0     28
    rear-9          8        4     21
    rear-12         8        4     21
    petzval-5      13        6     66
    plates-32      32        7    465

Measured (host build: clang++ 22, x86-64, CPU only; the paths are the same bare and coated).  `below`: the share of a lens's ghosts
whose f64 margin is below MARGIN, on the reference alone; errors: the largest absolute error of the ghosts both trace above the margin:

    lens       pairs  ghosts   traced   miss / clipped / TIR / turned     below     origin cm  dir       weight bare / film
    triplet-4    6     5 610    5 014       0 /    596 /     0 /   0     0.018 %   8.08e-7    5.99e-7   4.51e-9 / 3.29e-9
    fisheye-5   55    54 285   13 671  12 690 / 25 072 / 2 605 / 247     0.004 %   6.70e-4    7.58e-5   2.30e-8 / 8.67e-9
    mori-6      45    41 985   10 523      51 / 31 409 /     2 /   0     0.019 %   3.23e-6    6.41e-6   3.77e-9 / 9.91e-9
    double-3    55    53 845   26 145   1 558 / 22 088 / 4 054 /   0     0.019 %   4.95e-6    4.20e-6   4.01e-9 / 6.03e-9
    tessar-5    36    34 380   11 677       0 / 22 619 /    84 /   0     0.026 %   1.35e-6    1.26e-6   3.87e-9 / 2.70e-9
    petzval-2   28    25 732   10 395       0 / 15 337 /     0 /   0     0.004 %   3.85e-6    8.56e-7   3.16e-9 / 2.27e-9
    mori-4      28    27 440   10 338       0 / 17 102 /     0 /   0     0.044 %   2.36e-6    7.90e-6   4.21e-9 / 8.06e-9
    rear-9      21    20 223    3 212       0 / 15 101 / 1 887 /  23     0.015 %   3.97e-5    4.08e-6   3.07e-9 / 2.61e-9
    rear-12     21    20 664    3 946       0 / 14 797 / 1 921 /   0     0.034 %   4.53e-5    4.83e-6   3.35e-9 / 2.87e-9
    petzval-5   66    60 456   17 470       9 / 42 762 /   215 /   0     0.093 %   6.58e-6    6.56e-7   2.92e-9 / 2.33e-9
    plates-32  465    59 520   41 294       0 / 18 226 /     0 /   0     0.002 %   2.15e-6    8.26e-7   1.18e-9 / 1.16e-9

(the census is the host build's; the f64 restatement's differs from it on rear-9 only, by one ghost below the margin: TIR 1 886,
turned 24)

No ghost above the margin differs in reason, interface or leg; no dead record has a non-zero word.  CORPUS_MEASURED holds the largest
error of each quantity, CORPUS_PLAIN_MEASURED the plain path's (test_plain_path_is_the_strict_path; origin / dir against the host build
of trace_lens_spectral_strict, weight against the host build of path_transmittance):

    lens       starts that pass both   origin cm  dir       weight
    triplet-4  3 738  0.9997           4.98e-7    2.79e-7   1.19e-7
    fisheye-5  3 946  0.9997           6.68e-6    6.91e-7   1.79e-7
    mori-6     3 728  0.9989           9.84e-7    6.57e-7   2.09e-7
    double-3   3 908  0.9985           1.34e-6    3.54e-7   1.79e-7
    tessar-5   3 816  0.9995           5.36e-7    2.21e-7   1.19e-7
    petzval-2  3 669  0.9984           1.10e-6    1.63e-7   1.79e-7
    mori-4     3 915  0.9992           2.51e-7    3.02e-7   1.79e-7
    rear-9     3 494  0.9078           4.30e-5    2.64e-6   1.67e-6
    rear-12    3 759  0.9558           1.71e-5    1.90e-6   8.94e-7
    petzval-5  3 573  0.9760           1.04e-6    2.21e-7   2.38e-7
    plates-32  3 935  0.9982           5.94e-5    6.50e-7   1.34e-7

(plates-32's origin error is the STRICT trace's own: its plates are spheres of |R| = 3000 ... 3800, in the prescription's units, taken about their centres)

A wrong index is caught (scratch copies of ghost.hpp, host driver only, nothing committed):
  - leg 1's `G->surf[ii + 1].step` read as `S.step`: test_host_build_against_f64 fails on all eleven lenses, bare and coated (every lens
    has a pair with a non-empty leg 1): ghosts above the margin that differ in reason, interface or leg go from 0 to 275 (triplet-4),
    2 232 (plates-32), 2 901 (rear-9) ... 26 364 (mori-6); the origin error from 8.1e-7 ... 6.7e-4 cm to 0.15 ... 8.6 cm.  The plain
    path has no leg 1 and does not notice.
  - ghost_media's `cauchyB[i + 1]` read as `cauchyB[i]` (the wrong glass's dispersion in front of every interface):
    test_host_build_against_f64 and test_plain_path_is_the_strict_path fail on all eleven lenses (every glass has a V-number of its own):
    19 (triplet-4) ... 3 672 (petzval-5) ghosts differ, the weight error goes from 1.2e-9 ... 2.3e-8 to 1.3e-4 ... 6.8e-4, the plain
    path's from 1.2e-7 ... 1.7e-6 to 1.5e-2 and more.
  - both `i + 1` of ghost_media read as `i` (the medium in front taken for the one behind): every ghost ends as NO_REFLECTION, and both
    tests fail on all eleven lenses.
"""
import ctypes

import numpy as np
import pytest

import ghost_ref as gref
import lens_losses_corpus as lc
import machine_lens_corpus as mc
from fuzz_cameras import MachineLens
import host_drivers
from device_cases import bits_f32 as _bits
from ghost_ref import MARGIN, MAX_LEFT_OUT, bound as _bound, expected_pairs as _expected_pairs
from host_drivers import run_ghost_records as run_records, run_ghost_trace as run_trace, run_transmittance as run_transmittance_driver, split_ghost as split
from lens_losses_corpus import constructed as _constructed
from transmittance_ref import FILM_INDEX, FILM_LAMBDA0
from zoic_amd import ZoicCamera
from zoic_amd.camera import ZoicError

F32 = np.float32
# Host build against ghost_ref.ghost, every ghost both trace whose f64 margin is at least MARGIN, all pairs of all eleven lenses, bare and
# coated: the largest absolute error of the origin (cm), the direction and the weight (the table above); asserted: 4 x them, the
# project's margin for other compilers' host builds
CORPUS_MEASURED = dict(origin=6.698e-4, dir=7.581e-5, weight=2.303e-8)     # all three on fisheye-5, the weight bare
# Plain path from all of reference_rows, all eleven lenses
CORPUS_PLAIN_MEASURED = dict(origin=5.935e-5, dir=2.635e-6, weight=1.669e-6)     # origin on plates-32, dir and weight on rear-9
MIN_ROWS = 2048            # starts of a lens that pass at their wavelength in both host builds


@pytest.fixture(scope="module")
def driver():
    return host_drivers.ghost()


@pytest.fixture(scope="module")
def tdriver():
    return host_drivers.transmittance()


# ---- 1: the corpus -----------------------------------------------------------------------------------------------------------------
def test_the_corpus_is_the_pinned_one():
    """the texts by their crc32; per lens the interface count, the stop, the number of pairs and the equal-media interfaces; the pair
    list is the d-line rule; what this file rests on: counts 5 ... 14 and 32, the stop at 0 twice, NO_REFLECTION away from the stop on
    two lenses (see the module docstring), more than 32 pairs on at least three; 34 interfaces are refused"""
    for name in mc.NAMES:
        assert lc.crc(name) == mc.BY_NAME[name].crc, name
    assert lc.crc(lc.PLATES) == lc.PLATES_CRC and lc.PLATES not in mc.NAMES and len(lc.NAMES) == 11
    for name in lc.NAMES:
        T = lc.tables(name)
        assert (T["count"], T["stop"], len(T["pairs"]), T["equal"]) == lc.SHAPE[name], name
        assert np.array_equal(T["pairs"], _expected_pairs(T["disp"])), name
        reflecting = T["count"] - 1 - len(T["equal"])
        assert len(T["pairs"]) == reflecting * (reflecting - 1) // 2
        glass = T["disp"]["ior_d"] != 1
        assert len(set(T["disp"]["cauchy_b"][glass].tolist())) == glass.sum() >= 2, name      # every glass has a V-number of its own
    counts = {lc.SHAPE[n][0] for n in lc.NAMES}
    assert min(counts) == 5 and {14, 32} <= counts and len(counts) >= 8
    assert [n for n in lc.NAMES if lc.SHAPE[n][1] == 0] == ["mori-6", "mori-4"]
    assert {n: lc.SHAPE[n][3] for n in lc.NAMES if lc.SHAPE[n][3]} == {"fisheye-5": (6, 9), "petzval-2": (0,)}
    assert lc.SHAPE["fisheye-5"][0] == 14 and lc.SHAPE["fisheye-5"][2] == 11 * 10 // 2        # 11 of its 14 interfaces reflect
    assert sum(lc.SHAPE[n][2] > 32 for n in mc.NAMES) >= 3
    assert lc.SHAPE[lc.PLATES][0] == 32 and lc.SHAPE[lc.PLATES][2] == 465
    cam = ZoicCamera(device=-1)
    MachineLens(lc.plates_text(10)).load(cam)
    with pytest.raises(ZoicError) as e:
        cam.update(**mc.params("plates-34"))
    assert e.value.status_name == "ZOIC_ERR_TOO_MANY_LENSES"
    cam.close()


# ---- 2: the reference alone --------------------------------------------------------------------------------------------------------
_REFERENCE = {}


def _reference(oracle_lib, name):
    """ghost_ref.ghost of every pair of the lens from the f64 subset of its starts, bare and coated (the film changes the weight
    only): a list over the pairs of (bare, coated weight), the census and the share below the margin.  No library output is read."""
    if name not in _REFERENCE:
        T, S = lc.tables(name), lc.starts(oracle_lib, name)
        k = S["f64"]
        o, d, lam = S["o"][k], S["d"][k], S["lam"][k]
        per, seen, below = [], np.zeros(len(gref.REASONS), np.int64), 0
        for a, b in T["pairs"]:
            ref = gref.ghost(T["L"], T["disp"], lam, o, d, int(a), int(b))
            film = gref.ghost(T["L"], T["disp"], lam, o, d, int(a), int(b), *T["film"])
            assert np.array_equal(ref["reason"], film["reason"]) and np.array_equal(ref["origin"], film["origin"])
            per.append((ref, film["weight"]))
            seen += np.bincount(ref["reason"], minlength=len(seen))
            below += int((ref["margin"] < MARGIN).sum())
        total = len(o) * len(T["pairs"])
        _REFERENCE[name] = dict(per=per, seen=seen, below=below / total, ghosts=total, o=o, d=d, lam=lam)
    return _REFERENCE[name]


@pytest.mark.parametrize("name", lc.NAMES)
def test_reference_alone_meets_the_cap(oracle_lib, name):
    """on the f64 restatement alone: the share of ghosts whose margin is below MARGIN is at most MAX_LEFT_OUT; at least 1000 traced and
    100 clipped ghosts per lens"""
    R = _reference(oracle_lib, name)
    print("%-10s reference: ghosts %6d  below %.5f  %s" % (name, R["ghosts"], R["below"], dict(zip(gref.REASONS[:6], R["seen"][:6].tolist()))))
    assert R["below"] <= MAX_LEFT_OUT, (name, R["below"])
    assert R["seen"][gref.TRACED] >= 1000 and R["seen"][gref.CLIPPED] >= 100, (name, R["seen"])


def test_reference_alone_sees_every_reason(oracle_lib):
    """over the corpus MISS, CLIPPED, TIR and TURNED occur among the pairs of ghost_pairs(), and NO_REFLECTION on the pairs built on
    an equal-media interface or on the stop at index 0 -- the reference alone"""
    seen = sum(_reference(oracle_lib, name)["seen"] for name in lc.NAMES)
    for name in ("fisheye-5", "petzval-2", "mori-6", "mori-4"):
        T, R = lc.tables(name), _reference(oracle_lib, name)
        cases = _constructed(name)
        assert cases, name
        for a, b, reason, interface, leg in cases:
            ref = gref.ghost(T["L"], T["disp"], R["lam"], R["o"], R["d"], a, b)
            assert (ref["reason"] == reason).all() and (ref["interface"] == interface).all() and (ref["leg"] == leg).all(), (name, a, b)
            seen[reason] += len(R["o"])
    for why in (gref.TRACED, gref.MISS, gref.CLIPPED, gref.TIR, gref.TURNED, gref.NO_REFLECTION):
        assert seen[why] > 0, dict(zip(gref.REASONS, seen.tolist()))


# ---- 3: the host build against f64 ----------------------------------------------------------------------------------------------------
_AGAINST = {}


def _against(name, coated, driver, oracle_lib):
    key = (name, coated)
    if key not in _AGAINST:
        T, R = lc.tables(name), _reference(oracle_lib, name)
        got = run_records(driver, T["L"], T["disp"], R["lam"], R["o"], R["d"], T["pairs"], film=T["film"] if coated else None)
        err = dict(origin=0.0, dir=0.0, weight=0.0)
        wrong = 0
        seen = np.zeros(len(gref.REASONS), np.int64)
        for j, (ref, film_weight) in enumerate(R["per"]):
            go, gd, gw, flags, reason, iface, leg = split(got[:, j])
            sure = ref["margin"] >= MARGIN
            same = (reason == ref["reason"]) & (iface == ref["interface"]) & (leg == ref["leg"])
            wrong += int((sure & ~same).sum())
            seen += np.bincount(reason, minlength=len(seen))
            assert not _bits(got[:, j, :7][reason != 0]).any()                              # +0.0 everywhere
            both = sure & (reason == 0) & (ref["reason"] == 0)
            if both.any():
                want_w = film_weight if coated else ref["weight"]
                err["origin"] = max(err["origin"], float(np.abs(go[both] - ref["origin"][both]).max()))
                err["dir"] = max(err["dir"], float(np.abs(gd[both] - ref["dir"][both]).max()))
                err["weight"] = max(err["weight"], float(np.abs(gw[both] - want_w[both]).max()))
        _AGAINST[key] = dict(err=err, wrong=wrong, seen=seen, records=got)
        print("%-10s %-5s pairs %3d ghosts %6d  %s  below %.5f  wrong %d  origin %.3e dir %.3e weight %.3e" % (
            name, "film" if coated else "bare", len(T["pairs"]), R["ghosts"], " / ".join("%d" % v for v in seen[:5]), R["below"], wrong,
            err["origin"], err["dir"], err["weight"]))
    return _AGAINST[key]


@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_host_build_against_f64(name, coated, driver, oracle_lib):
    """every pair of ghost_pairs(), bare and with a film where the media differ: reason, interface and leg equal for every ghost whose
    f64 margin is at least MARGIN (the reference alone keeps the share below it under MAX_LEFT_OUT, asserted first); dead records
    +0.0; origin, dir and weight of the ghosts both trace within 4 x CORPUS_MEASURED.  The table is in the module docstring."""
    R = _reference(oracle_lib, name)
    assert R["below"] <= MAX_LEFT_OUT
    m = _against(name, coated, driver, oracle_lib)
    assert m["wrong"] == 0, (name, m["wrong"])
    bound = _bound(CORPUS_MEASURED)
    for k in ("origin", "dir", "weight"):
        assert m["err"][k] <= bound[k], (name, k, m["err"][k])
    assert m["seen"][gref.TRACED] >= 1000 and m["seen"][gref.CLIPPED] >= 100, m["seen"]


def test_corpus_measured_is_the_measured_one(driver, oracle_lib):
    for k in ("origin", "dir", "weight"):
        worst = max(_against(name, coated, driver, oracle_lib)["err"][k] for name in lc.NAMES for coated in (False, True))
        assert CORPUS_MEASURED[k] / 4 <= worst <= 4 * CORPUS_MEASURED[k], (k, worst)


@pytest.mark.parametrize("name", lc.NAMES)
def test_traced_records(name, driver, oracle_lib):
    """every traced ghost of the runs above: 0 < weight <= 1, unit dir with dir.z < 0 in the record frame, origin on the front cap
    within its housing (test_ghost_cpu.test_traced_records on a corpus lens)"""
    L = lc.tables(name)["L"]
    for coated in (False, True):
        rec = _against(name, coated, driver, oracle_lib)["records"].reshape(-1, 8)
        rec = rec[_bits(rec[:, 7]) == 1].astype(np.float64)
        assert len(rec) >= 1000
        w = rec[:, 6]
        assert (w > 0).all() and (w <= 1).all()
        assert (rec[:, 5] < 0).all() and np.abs(np.linalg.norm(rec[:, 3:6], axis=1) - 1).max() <= 1e-5
        R, zv = float(L["radius"][-1]), float(L["vertex"][-1])
        p = -rec[:, 0:3]                                            # trace frame
        assert (p[:, 0] ** 2 + p[:, 1] ** 2 <= float(L["housing2"][-1])).all()
        on_sphere = np.abs(np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2 + (p[:, 2] - (zv - R)) ** 2) - abs(R))
        assert on_sphere.max() <= 1e-5 * max(1.0, abs(zv), abs(R)) + 4 * _bound(CORPUS_MEASURED)["origin"], on_sphere.max()
        assert (np.sign(R) * (p[:, 2] - (zv - R)) > 0).all()        # the vertex-side cap


# ---- 4: the plain path ---------------------------------------------------------------------------------------------------------------
_PLAIN = {}


def _plain(name, driver, tdriver, oracle_lib):
    """"no pair" from all of reference_rows against the host builds of trace_lens_spectral_strict and path_transmittance:
    test_ghost_cpu._plain's comparison and disagreement rule on a corpus lens"""
    if name not in _PLAIN:
        T, S = lc.tables(name), lc.starts(oracle_lib, name)
        L, disp, surf = T["L"], T["disp"], T["surf"]
        o, d, lam = S["o"], S["d"], S["lam"]
        got = run_trace(driver, L, disp, lam, o, d, -1, -1)
        go, gd, gw, flags, _, _, _ = split(got)
        s4 = np.ascontiguousarray(np.stack([surf[:, 0], surf[:, 1], surf[:, 2], T["housing2"]], 1), F32)
        dp = np.ascontiguousarray(np.stack([disp["ior_d"], disp["cauchy_b"]], 1), F32)
        fp = ctypes.POINTER(ctypes.c_float)
        o32, d32, l32 = (np.ascontiguousarray(v, F32) for v in (o, d, lam))
        ref = np.zeros((len(o), 7), F32)
        driver.zgh_strict(len(surf), s4.ctypes.data_as(fp), dp.ctypes.data_as(fp), len(o), l32.ctypes.data_as(fp), o32.ctypes.data_as(fp),
                          d32.ctypes.data_as(fp), ref.ctypes.data_as(fp))
        passes, traced = ref[:, 6] != 0, flags == 1
        margin = gref.ghost(L, disp, lam, o, d, -1, -1)["margin"]
        # the two may differ on a ray that STRICT's rounding decides (test_ghost_cpu._plain has the estimate): beyond that margin of the
        # f64 path they must agree
        assert np.array_equal(passes[margin >= 5e-3], traced[margin >= 5e-3]) and (passes != traced).mean() <= 1e-3, name
        both = passes & traced
        assert both.sum() >= MIN_ROWS, (name, int(both.sum()))
        ro, rd = ref[both, 0:3].astype(np.float64), ref[both, 3:6].astype(np.float64)
        rd /= np.linalg.norm(rd, axis=1, keepdims=True)
        t = run_transmittance_driver(tdriver, surf, disp, lam, o, d, None, T["housing2"])
        assert np.array_equal(t != 0, passes)                      # path_transmittance passes where the STRICT trace does
        _PLAIN[name] = dict(origin=float(np.abs(-go[both].astype(np.float64) - ro).max()), dir=float(np.abs(-gd[both].astype(np.float64) - rd).max()),
                            weight=float(np.abs(gw.astype(np.float64) - t)[both].max()), rows=int(both.sum()), share=float(both.mean()))
        print("%-10s plain path: rows %4d (%.4f of the starts)  origin %.3e dir %.3e weight %.3e" % (
            name, _PLAIN[name]["rows"], _PLAIN[name]["share"], _PLAIN[name]["origin"], _PLAIN[name]["dir"], _PLAIN[name]["weight"]))
    return _PLAIN[name]


@pytest.mark.parametrize("name", lc.NAMES)
def test_plain_path_is_the_strict_path(name, driver, tdriver, oracle_lib):
    """ghost_trace(-1, -1) from every start: exit origin and unit direction against the host build of trace_lens_spectral_strict, the
    weight against the host build of path_transmittance, within 4 x CORPUS_PLAIN_MEASURED; the two traces pass the same starts beyond
    a margin of 5e-3 and disagree on at most 1 in 1000; at least MIN_ROWS starts pass both"""
    m = _plain(name, driver, tdriver, oracle_lib)
    bound = _bound(CORPUS_PLAIN_MEASURED)
    for k in ("origin", "dir", "weight"):
        assert m[k] <= bound[k], (name, k, m[k])


def test_corpus_plain_measured_is_the_measured_one(driver, tdriver, oracle_lib):
    for k in ("origin", "dir", "weight"):
        worst = max(_plain(name, driver, tdriver, oracle_lib)[k] for name in lc.NAMES)
        assert CORPUS_PLAIN_MEASURED[k] / 4 <= worst <= 4 * CORPUS_PLAIN_MEASURED[k], (k, worst)


# ---- 5: equal media and the stop at index 0, by construction -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fisheye-5", "petzval-2", "mori-6", "mori-4"])
def test_no_reflection_away_from_the_middle_stop(name, driver, oracle_lib):
    """a on an equal-media interface that is not the stop: NO_REFLECTION there on leg 0; b on one: NO_REFLECTION there on leg 1; the
    stop at trace index 0: every pair (a, 0) gives NO_REFLECTION, interface 0, leg 1.  Every start, the documented flag word, +0.0 in
    the seven floats, bare and coated."""
    T, S = lc.tables(name), lc.starts(oracle_lib, name)
    cases = _constructed(name)
    assert {c[4] for c in cases} == ({0, 1} if name == "fisheye-5" else {1})
    if name in ("mori-6", "mori-4"):
        assert T["stop"] == 0 and len(cases) == T["count"] - 1
    for film in (None, T["film"]):
        got = run_records(driver, T["L"], T["disp"], S["lam"], S["o"], S["d"], [c[:2] for c in cases], film=film)
        for j, (a, b, reason, interface, leg) in enumerate(cases):
            assert (_bits(got[:, j, 7]) == gref.flag_word(reason, interface, leg)).all(), (name, a, b)
            assert not _bits(got[:, j, :7]).any()


@pytest.mark.parametrize("name", ["mori-6", "mori-4"])
def test_no_ghost_crosses_a_stop_at_index_0(name, driver, oracle_lib):
    """the stop at trace index 0: leg 0 starts on it, no leg 1 reaches it (b >= 1) and leg 2 starts beyond it, so no ghost of the pair
    list ends on interface 0 on leg 1 or 2; a ghost clipped by the stop is clipped on leg 0"""
    T = lc.tables(name)
    assert (T["pairs"][:, 1] >= 1).all()
    for coated in (False, True):
        rec = _against(name, coated, driver, oracle_lib)["records"]
        _, _, _, flags, reason, iface, leg = split(rec)
        dead = reason != 0
        assert not (dead & (iface == 0) & (leg != 0)).any()


def test_a_leg_across_equal_media_leaves_the_weight_alone(driver, oracle_lib):
    """fisheye-5, the pair (11, 7): all three legs cross interface 9, between equal media (air on both sides).  The refraction there
    takes eta == 1 and leaves the weight alone: the weight is the f64 weight, in which that interface's factor is exactly 1, within
    4 x CORPUS_MEASURED, and a film on that interface (and on the other equal-media interface and the stop) changes no word of any
    record.  The same on the pair (7, 2), whose leg 1 crosses interface 6 and the stop."""
    name = "fisheye-5"
    T, R = lc.tables(name), _reference(oracle_lib, name)
    assert T["equal"] == (6, 9) and T["stop"] == 5
    pairs = np.array([(11, 7), (7, 2)])
    index = {tuple(p): j for j, p in enumerate(T["pairs"].tolist())}
    everywhere = (np.full(T["count"], FILM_INDEX, F32), np.full(T["count"], FILM_LAMBDA0, F32))
    assert (T["film"][0][[5, 6, 9]] == 0).all()
    some = run_records(driver, T["L"], T["disp"], R["lam"], R["o"], R["d"], pairs, film=T["film"])
    every = run_records(driver, T["L"], T["disp"], R["lam"], R["o"], R["d"], pairs, film=everywhere)
    assert np.array_equal(_bits(some), _bits(every))
    traced = 0
    for j, pair in enumerate(pairs.tolist()):
        ref, film_weight = R["per"][index[tuple(pair)]]
        go, gd, gw, flags, reason, iface, leg = split(some[:, j])
        both = (ref["margin"] >= MARGIN) & (reason == 0) & (ref["reason"] == 0)
        traced += int(both.sum())
        assert np.abs(gw[both] - film_weight[both]).max() <= _bound(CORPUS_MEASURED)["weight"]
        assert not (reason == gref.TIR)[iface == (9 if j == 0 else 6)].any()       # eta == 1: no total reflection there
    assert traced >= 100, traced

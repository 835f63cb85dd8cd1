"""The backward paths on the pinned corpus of machine-made lenses (machine_lens_corpus.py), without a GPU: the host builds of
csrc/traceback.hpp, csrc/reverse.hpp and csrc/backward_spectral.hpp (zoic_trace_back_ray, zoic_project_point and their spectral
siblings on tables-only cameras) against the f64 restatements traceback_ref.py and backward_spectral_ref.py.

Inputs.  Every lens sits behind fuzz_cameras.EXAMPLE_CAMERA (sensorHeight 2.0, no image).  Trace-back: the oracle's d-line records of
weight > 0 on the 192 x 108 x 2 frame of traceback_cases (41 472 rays), taken back at the d-line, 400, 486.1327, 656.2725 and 700 nm;
projection: reverse_ref.kolb_point_set.  Edge rays (TraceBack.edge: 1e-2 at the stop, 1e-4 elsewhere) are left out.

The six ACCURACY lenses meet the reference-only conditions (edge share <= 2 %, >= 4096 non-edge records the f64 trace takes back, the
f64 projection finds >= 99 % of the point set) on the full frame at all five wavelengths, asserted from the restatements alone before
the library is looked at: no lens of the list was replaced.  Measured on the full frame and the full point sets:

    lens        live    edge share % (d / 400 / 486 / 656 / 700)   least non-edge traced   points   ok_ref
    triplet-4   25 406   0.00 / 0.04 / 0.02 / 0.01 / 0.01           25 339 (400 nm)         16 384   1.000
    fisheye-5   41 468   0.94 / 0.95 / 0.96 / 1.05 / 1.05           38 699 (400 nm)         16 384   1.000
    mori-6      32 576   0.06 / 0.02 / 0.06 / 0.07 / 0.07           32 089 (400 nm)          1 104   1.000
    double-3    41 472   0.78 / 0.00 / 0.12 / 1.11 / 1.25           40 894 (700 nm)         16 384   1.000
    tessar-5    22 675   0.26 / 0.18 / 0.21 / 0.27 / 0.27           22 576 (400 nm)          9 040   1.000
    petzval-2   16 413   0.46 / 0.55 / 0.48 / 0.46 / 0.42           16 189 (700 nm)          3 616   1.000

The d-line trace-back is held to traceback_cpu's bounds: |library - f64| max and p99 <= 4 x E_ref (E_ref = |Ps of the f64 trace-back -
the sample the record was made from|, the forward path's own noise), round trip <= 5 x max E_ref.  The spectral calls are held to
backward_spectral_cpu's: each wavelength's max |library - f64| <= 2 x the same lens's d-line max.  Measured:

    lens        E_ref max / p99      |lib - f64| / E_ref (max / p99)   round trip / max E_ref
    triplet-4   7.13e-7 / 3.54e-7    0.61 / 0.62                       1.00
    fisheye-5   1.82e-6 / 8.62e-7    1.46 / 1.45                       2.07
    mori-6      1.98e-6 / 1.13e-6    0.49 / 0.43                       1.09
    double-3    1.24e-6 / 6.53e-7    0.73 / 0.76                       1.39
    tessar-5    9.82e-7 / 4.92e-7    0.60 / 0.65                       0.97
    petzval-2   4.94e-7 / 3.07e-7    0.72 / 0.62                       1.16

    max |library - f64|   trace-back: d-line, then / d-line at 400, 486, 656, 700   projection: d-line, then / d-line at 400, 486, 656, 700
    triplet-4             4.37e-7   0.96  1.03  1.13  0.94                            5.64e-7   0.80  0.92  0.85  0.83
    fisheye-5             2.65e-6   1.04  0.85  1.25  0.80                            1.09e-6   1.01  1.04  0.99  0.96
    mori-6                9.76e-7   1.12  1.15  0.97  0.90                            4.79e-7   0.76  0.66  1.11  0.83
    double-3              9.13e-7   1.23  1.13  1.25  1.09                            5.60e-7   1.08  1.05  0.84  1.00
    tessar-5              5.90e-7   1.13  0.85  0.92  1.04                            3.47e-7   1.36  0.88  1.04  1.29
    petzval-2             3.57e-7   1.07  0.96  0.95  0.93                            1.39e-7   1.32  1.60  1.47  1.96

(petzval-2's projection errs by one or two ulps of a sample near 1: 1.39e-7 at the d-line, 2.72e-7 at 700 nm.)

The BITWISE lenses carry no error bound and no edge cap: decisions equal to the f64 trace's off the edge set, reasons and interface
indices equal off decision_edge, at the d-line, 400 and 700 nm.  Mismatches: none.  Their edge shares and (not bounded) errors:

    lens      live     edge share % (d / 400 / 700)   max |lib - f64| (d / 400 / 700)   points   projected: f64 / library
    mori-4    18 461   0.02 / 0.02 / 0.01             6.2e-7 / 6.6e-7 / 5.2e-7           1 264   1.000 / 1.000
    rear-9    23 947   1.45 / 0.00 / 2.77             1.7e-5 / 1.1e-4 / 9.8e-6           1 872   1.000 / 1.000
    rear-12   38 949   1.09 / 0.02 / 2.08             4.2e-6 / 8.0e-6 / 5.1e-6           5 360   1.000 / 1.000
    petzval-5 outside the geometric domain (fastRunsStrict): 11 189 live forward records; every one of 8 834 rays is refused
              kTbOutsideDomain (7) and every one of 1 814 points kRevOutsideDomain (5), at the d-line, 400 and 700 nm, Ps = (+0, +0)

On every lens the rays made to be refused (rejection families of live records, random lines, non-finite rays: ~5000) end for all of
the reasons 1 ... 5, and the spectral calls at 587.5618 nm give the d-line calls' bits.
"""
import numpy as np
import pytest

from zoic_amd import _capi

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import traceback_cases as tc
from device_cases import bits as _bits
from machine_lens_corpus import EDGE_CAP
from traceback_cases import lib_project, lib_trace
from traceback_ref import CLIPPED, MISS, OUTSIDE_DOMAIN, TIR

REV_OUTSIDE = 5                       # kRevOutsideDomain (csrc/reverse.hpp)
F32 = np.float32
WAVELENGTHS = (None,) + bs.LAMBDAS    # None: the d-line calls and the d-line restatement
BITWISE_WAVELENGTHS = (None, 400.0, 700.0)


def _tag(lam):
    return "d" if lam is None else "%g" % lam


class _Lens:
    """one corpus lens: its tables-only camera, the live oracle records of the frame and the f64 restatements of both paths, each
    computed once and shared by the tests below"""

    def __init__(self, oracle_lib, name):
        self.name = name
        self.cam, self.p = mc.camera(name)
        self.info, self.disp = self.cam.info(), self.cam.dispersion()
        self.T = bs.SpectralTraceBack(self.info, self.p, self.disp)
        s, o, d, w = mc.oracle_records(oracle_lib, name)
        live = w > 0
        self.o, self.d, self.smp = o[live], d[live], s[live, :2].astype(np.float64)
        self.pts = mc.point_set(name)[0]
        self._tb, self._pp = {}, {}

    def trace(self, lam):
        """the f64 trace-back of the live records at one wavelength and its edge set"""
        if lam not in self._tb:
            ref = self.T.trace(self.o, self.d) if lam is None else self.T.trace_at(self.o, self.d, lam)
            self._tb[lam] = ref, self.T.edge(ref)
        return self._tb[lam]

    def project(self, lam):
        """the f64 projection of the point set at one wavelength: (ps, ok)"""
        if lam not in self._pp:
            self._pp[lam] = bs.project_at(self.info, self.p["sensorWidth"], self.disp, self.pts, bs.LAMBDA_D if lam is None else lam)
        return self._pp[lam]


_LENSES = {}


def _lens(oracle_lib, name):
    if name not in _LENSES:
        _LENSES[name] = _Lens(oracle_lib, name)
    return _LENSES[name]


# ---- 0. the corpus itself ----------------------------------------------------------------------------------------------------------
def test_the_corpus_is_the_pinned_one():
    for e in mc.CORPUS:
        assert mc.crc(e.name) == e.crc, "%s: the generated prescription changed (crc32 0x%08x, pinned 0x%08x)" % (e.name, mc.crc(e.name), e.crc)
        cam, p = mc.camera(e.name)
        info = cam.info()
        print("%-10s crc32 0x%08x  interfaces %2d  stop at trace index %d  fastRunsStrict %s" % (
            e.name, mc.crc(e.name), info["lensCount"], info["apertureElement"], bool(info["fastRunsStrict"])))
        assert info["lensCount"] == e.interfaces, (e.name, info["lensCount"])
        assert bool(info["fastRunsStrict"]) == (e.name == mc.OUTSIDE), e.name
        if e.name.startswith("mori"):
            assert info["apertureElement"] == 0, (e.name, info["apertureElement"])
        assert cam.dispersion()["cauchy_b"].any(), e.name     # every lens has colour
        cam.close()
    assert len(mc.ACCURACY) == 6 and len(mc.BITWISE) == 4
    counts = [e.interfaces for e in mc.CORPUS]
    assert min(counts) == 5 and max(counts) == 14


# ---- 1. the conditions an accuracy lens meets by the restatement alone ------------------------------------------------------------
@pytest.mark.parametrize("name", mc.ACCURACY)
def test_reference_only_conditions(oracle_lib, name):
    """Asserted on the f64 restatements alone, before the library is looked at: the edge share of the frame's live records, the number
    of non-edge records the f64 trace takes back, and the share of the point set the f64 projection finds, at every wavelength."""
    L = _lens(oracle_lib, name)
    for lam in WAVELENGTHS:
        ref, edge = L.trace(lam)
        traced = int((ref["traced"] & ~edge).sum())
        ok_ref = L.project(lam)[1]
        print("%s %8s: live %d, edge share %.2f %%, non-edge traced %d; projection: %d points, ok_ref %.4f" % (
            name, _tag(lam), len(edge), 100 * edge.mean(), traced, len(L.pts), ok_ref.mean()))
        assert edge.mean() <= EDGE_CAP, (lam, edge.mean())
        assert traced >= 4096, (lam, traced)
        assert len(L.pts) >= 1000 and ok_ref.mean() >= 0.99, (lam, len(L.pts), ok_ref.mean())


# ---- 2. the d-line trace-back against the f64 trace, the forward path's own noise the yardstick ---------------------------------
def _refusals(L):
    """rays a trace-back refuses for every reason: the rejection families of a stride of live records, random lines, non-finite rays"""
    pick = np.flatnonzero(~L.trace(None)[1])
    pick = mc.strided(pick, 1024)
    fam = tc.rejection_families(L.info, L.o[pick], L.d[pick])
    sets = list(fam.values()) + [tc.random_lines(L.info, 1024), tc.non_finite_rays()]
    return np.concatenate([o for o, _ in sets]).astype(F32), np.concatenate([d for _, d in sets]).astype(F32)


def _decisions(L, o, d, lam, ref=None, edge=None):
    """decisions equal to the f64 trace's off the edge set; reasons and interface indices equal off decision_edge; a refused ray
    gives (+0, +0).  Returns (ps, flags, mismatches counted for the print)."""
    if ref is None:
        ref = L.T.trace(o, d) if lam is None else L.T.trace_at(o, d, lam)
        edge = L.T.edge(ref)
    ps, fl = lib_trace(L.cam, o, d, lam)
    ok = (fl & 1) == 1
    assert np.array_equal(ok[~edge], ref["traced"][~edge]), (L.name, lam, int((ok[~edge] != ref["traced"][~edge]).sum()))
    keep = ~L.T.decision_edge(ref)
    no = keep & ~ok
    assert np.array_equal(tc.reason(fl[no]), ref["reason"][no]), (L.name, lam)
    ended = no & np.isin(ref["reason"], (MISS, CLIPPED, TIR))
    assert np.array_equal(tc.iface(fl[ended]), ref["iface"][ended]), (L.name, lam)
    assert (ps[~ok].view(np.uint32) == 0).all(), (L.name, lam)
    return ps, fl, ok, ref, edge


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_trace_back_accuracy(oracle_lib, name):
    L = _lens(oracle_lib, name)
    ref, edge = L.trace(None)
    good = ~edge & ref["traced"]
    e_ref = np.abs(ref["ps"] - L.smp).max(1)[good]
    e_max, e_p99 = float(e_ref.max()), float(np.percentile(e_ref, 99))
    ps, fl, ok, _, _ = _decisions(L, L.o, L.d, None, ref, edge)
    both = good & ok
    err = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
    rt = np.abs(ps.astype(np.float64) - L.smp).max(1)[both]
    print("%s: live %d, non-edge traced %d, E_ref max %.3g p99 %.3g; |lib - f64| max %.3g p99 %.3g (%.2f / %.2f of E_ref); round trip max %.3g "
          "(%.2f of max E_ref)" % (name, len(edge), both.sum(), e_max, e_p99, err.max(), np.percentile(err, 99), err.max() / e_max,
                                   np.percentile(err, 99) / e_p99, rt.max(), rt.max() / e_max))
    assert both.sum() >= 4096
    assert err.max() <= 4.0 * e_max, (err.max(), e_max)
    assert np.percentile(err, 99) <= 4.0 * e_p99, (np.percentile(err, 99), e_p99)
    assert rt.max() <= 5.0 * e_max, (rt.max(), e_max)
    # what it must refuse, and why
    o, d = _refusals(L)
    _, rfl, rok, rref, _ = _decisions(L, o, d, None)
    seen = sorted(set(tc.reason(rfl[~rok]).tolist()))
    print("%s: %d rays made to be refused, %d refused, reasons %s" % (name, len(o), (~rok).sum(), seen))
    assert len(seen) >= 4, seen


# ---- 3. the spectral calls ---------------------------------------------------------------------------------------------------------
def _tb_error(L, lam):
    """max and p99 of |library - f64| over the non-edge records both take back at one wavelength"""
    ref, edge = L.trace(lam)
    ps, fl, ok, _, _ = _decisions(L, L.o, L.d, lam, ref, edge)
    both = ~edge & ok & ref["traced"]
    assert both.sum() >= 4096
    err = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
    return float(err.max()), float(np.percentile(err, 99))


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_spectral_trace_back_accuracy(oracle_lib, name):
    L = _lens(oracle_lib, name)
    d_max, d_p99 = _tb_error(L, None)
    print("%s trace-back   d-line : max %.3g p99 %.3g" % (name, d_max, d_p99))
    for lam in bs.LAMBDAS:
        e_max, e_p99 = _tb_error(L, lam)
        print("%s trace-back %8.4f : max %.3g p99 %.3g  (%.2f of the d-line max)" % (name, lam, e_max, e_p99, e_max / d_max))
        assert e_max <= 2.0 * d_max, (lam, e_max, d_max)


def _proj_error(L, lam):
    ref, ok_ref = L.project(lam)
    ps, fl = lib_project(L.cam, L.pts, lam)
    ok = (fl & 1) == 1
    assert ok_ref.mean() >= 0.99 and ok[ok_ref].all(), (L.name, lam, ok_ref.mean(), ok.mean())
    err = np.abs(ps.astype(np.float64) - ref).max(1)[ok & ok_ref]
    return float(err.max()), float(np.percentile(err, 99))


@pytest.mark.parametrize("name", mc.ACCURACY)
def test_spectral_projection_accuracy(oracle_lib, name):
    L = _lens(oracle_lib, name)
    d_max, d_p99 = _proj_error(L, None)
    print("%s projection   d-line : max %.3g p99 %.3g (%d points)" % (name, d_max, d_p99, len(L.pts)))
    for lam in bs.LAMBDAS:
        e_max, e_p99 = _proj_error(L, lam)
        print("%s projection %8.4f : max %.3g p99 %.3g  (%.2f of the d-line max)" % (name, lam, e_max, e_p99, e_max / d_max))
        assert e_max <= 2.0 * d_max, (lam, e_max, d_max)


@pytest.mark.parametrize("name", mc.NAMES)
def test_d_line_bits_and_rejected_wavelengths(oracle_lib, name):
    """at 587.5618 nm the spectral calls give the d-line calls' bits; a rejected wavelength is reported before anything else (before
    the domain gate of the lens outside the domain too)"""
    L = _lens(oracle_lib, name)
    ro, rd = _refusals(L)
    o = np.concatenate([mc.strided(L.o, 2048).astype(F32), ro])
    d = np.concatenate([mc.strided(L.d, 2048).astype(F32), rd])
    ps0, fl0 = lib_trace(L.cam, o, d)
    ps1, fl1 = lib_trace(L.cam, o, d, bs.LAMBDA_D)
    assert np.array_equal(fl0, fl1) and np.array_equal(_bits(ps0), _bits(ps1))
    pts = mc.strided(L.pts, mc.MAX_POINTS) if len(L.pts) else mc.strided(mc.point_set("petzval-2")[0], mc.MAX_POINTS)
    qs0, gl0 = lib_project(L.cam, pts)
    qs1, gl1 = lib_project(L.cam, pts, bs.LAMBDA_D)
    assert np.array_equal(gl0, gl1) and np.array_equal(_bits(qs0), _bits(qs1))
    if name != mc.OUTSIDE:
        assert (fl0 & 1).sum() >= 1000 and ((fl0 & 1) == 0).sum() >= 100 and (gl0 & 1).mean() >= 0.9
    lam = np.resize(np.array(bs.REJECTED, F32), len(o))
    ps, fl = lib_trace(L.cam, o, d, lam)
    assert (fl == _capi.TRACE_BACK_WAVELENGTH << 8).all() and not _bits(ps).any()
    lam = np.resize(np.array(bs.REJECTED, F32), len(pts))
    qs, gl = lib_project(L.cam, pts, lam)
    assert (gl == _capi.PROJECT_WAVELENGTH << 8).all() and not _bits(qs).any()


# ---- 4. the lenses held to decisions only ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in mc.BITWISE if n != mc.OUTSIDE])
def test_bitwise_only_lenses_decide_as_the_f64_trace(oracle_lib, name):
    """No error bound and no edge cap: the edge set only takes rays out of the comparison of decisions, and its share is printed."""
    L = _lens(oracle_lib, name)
    o, d = _refusals(L)
    for lam in BITWISE_WAVELENGTHS:
        ref, edge = L.trace(lam)
        ps, fl, ok, _, _ = _decisions(L, L.o, L.d, lam, ref, edge)
        both = ~edge & ok
        err = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
        _, rfl, rok, rref, redge = _decisions(L, o, d, lam)
        ref_p, ok_ref = L.project(lam)
        qs, gl = lib_project(L.cam, L.pts, lam)
        print("%s %8s: live %d, edge share %.2f %%, traced back %d (|lib - f64| max %.3g, not bounded); %d rays made to be refused, edge share "
              "%.2f %%, reasons %s; projection: %d points, ok_ref %.4f, library %.4f" % (
                  name, _tag(lam), len(edge), 100 * edge.mean(), both.sum(), err.max() if len(err) else 0.0, len(o), 100 * redge.mean(),
                  sorted(set(tc.reason(rfl[~rok]).tolist())), len(L.pts), ok_ref.mean() if len(ok_ref) else 0.0, (gl & 1).mean() if len(gl) else 0.0))
        assert both.sum() >= 1024, (lam, both.sum())
        assert ((gl & 1) == 1)[ok_ref].all(), (lam, int((((gl & 1) == 0) & ok_ref).sum()))   # what the f64 projection finds, the library projects
        seen = set(tc.reason(rfl[~rok]).tolist())
        assert len(seen) >= 4, (lam, seen)


def test_the_lens_outside_the_domain_refuses_everything(oracle_lib):
    L = _lens(oracle_lib, mc.OUTSIDE)
    assert L.info["fastRunsStrict"]
    ro, rd = _refusals(L)
    o = np.concatenate([mc.strided(L.o, 4096).astype(F32), ro])
    d = np.concatenate([mc.strided(L.d, 4096).astype(F32), rd])
    nan, inf = F32(np.nan), F32(np.inf)
    pts = np.concatenate([mc.strided(mc.point_set("petzval-2")[0], mc.MAX_POINTS),
                          np.array([[0.1, 0.2, 1.0], [nan, 0, -10], [0, inf, -10], [0, 0, -5], [-0.0, -0.0, -5], [3, 1, -1e30]], F32)])
    print("%s: %d live records of the forward (STRICT) path, %d rays and %d points refused" % (mc.OUTSIDE, len(L.o), len(o), len(pts)))
    assert len(L.o) >= 1024
    for lam in BITWISE_WAVELENGTHS:
        ps, fl = lib_trace(L.cam, o, d, lam)
        assert (fl == OUTSIDE_DOMAIN << 8).all() and not _bits(ps).any(), lam
        ref = L.T.trace(o, d) if lam is None else L.T.trace_at(o, d, lam)
        assert (ref["reason"] == OUTSIDE_DOMAIN).all() and not ref["traced"].any()
        qs, gl = lib_project(L.cam, pts, lam)
        assert (gl == REV_OUTSIDE << 8).all() and not _bits(qs).any(), lam

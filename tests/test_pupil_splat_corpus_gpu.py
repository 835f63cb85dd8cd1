"""Pupil bounds and lens splats on the MI355X over the pinned corpus of machine-made lenses (machine_lens_corpus.py: 5 ... 14
interfaces, the stop at trace index 0, near-hemispherical rear elements, a V column, a lens outside the geometric domain), after
tests/test_pupil_splat_corpus_cpu.py, which holds the host twins (csrc/pupil_bounds.hpp and csrc/splat.hpp compiled for the host) to
independent restatements and to the f64 trace.  Every comparison here is bitwise against those twins, on STRICT cameras.

Points, wavelengths and u: pupil_splat_corpus.py (at most 71 points a lens, bs.mixed_wavelengths: a rejected wavelength at every
fourth point, so the four waves of a pupil-bounds workgroup and the lanes of a splat wave differ).  The points are given to the device
in pupil_splat_corpus.device_order: a single-lane row (fisheye-5: the whole pupil is one lattice aim, held by one lane of the wave's
butterfly), the sparsest rows and two rows with count >= 64 come first, so the prefixes n = 1, 3, 4, 5 hold them.

  * pupil bounds, all ten lenses: lattices 8, 16 and 32 without a window and 16 with pupil_cases.WINDOW, d-line and mixed wavelengths,
    the whole set and its prefixes of 1, 3, 4 and 5 points; fisheye-5 and triplet-4 (the most and the fewest interfaces) also
    4 x 2048 + 1 points at lattice 8, the set tiled: the grid-stride walk's second slab;
  * splats, all ten lenses: the bounds come from the device call on the same stream and are read in place; (n, m) = (1, 1), (3, 5),
    (5, 64), (2, 257) and (the whole set, 7), d-line and mixed wavelengths; fisheye-5 and triplet-4 also 2^19 + 1 splats with m = 3,
    the set tiled; a forced box on petzval-5; sx, sy and the flag word of every traced or refused splat are cam.trace_back's on
    the same rays;
  * one camera, one `out` buffer for the bounds and one for the splats, updated from double-3 to fisheye-5 to petzval-5 with no
    reallocation: after each update every record is the new lens's and nothing past n (n m) is written;
  * at 587.5618 nm the spectral kernels give the d-line kernels' bits on every lens.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_STRICT, ZoicCamera, _capi, pupil_bounds_records, splat_records

import backward_spectral_ref as bs
import machine_lens_corpus as mc
import pupil_driver
import pupil_ref
import pupil_splat_corpus as psc
import splat_driver
import splat_ref
from device_cases import bits as _bits, records as _records
from traceback_ref import OUTSIDE_DOMAIN

F32 = np.float32
PREFIXES = (1, 3, 4, 5)
GRID_CAP = 2048                      # workgroups a launch is capped at (kPassGridCap, device_pass.hpp; pupil_bounds.hip: four points each; splat.hip: 256 splats each)
SLAB_PLUS_ONE = 4 * GRID_CAP + 1     # pupil bounds: one slab of the grid-stride walk and one point
STRIDE_SHAPE = (174763, 3)           # splats: 2^19 + 1 = 3 x 174763
assert STRIDE_SHAPE[0] * STRIDE_SHAPE[1] == GRID_CAP * 256 + 1
SPLAT_SHAPES = ((1, 1), (3, 5), (5, 64), (2, 257))
CONFIGS = ((8, None), (16, None), (32, None), (16, psc.WINDOW))
G = psc.SPLAT_LATTICE


def _camera(name):
    cam, p = mc.camera(name, device=0, precision=PRECISION_STRICT)
    return cam, dict(p, useDof=True)


def _host_bounds(cam, p, pts, lattice, window=None, lam=None):
    return pupil_driver.drive_pupil(pupil_driver.pupil(), cam, p, pts, lattice, window, lam, None if lam is None else cam.dispersion())


def _host_splats(cam, p, pts, bounds, u, lam=None):
    return splat_driver.drive_splat(splat_driver.splat(), cam, p, pts, bounds, u, lam, None if lam is None else cam.dispersion())


def _ordered(name, lattice):
    """(points in device order, wavelengths by position, the restatement's passing mask in that order)"""
    order = psc.device_order(name, lattice)
    pts = np.ascontiguousarray(psc.points(name)[0][order])
    return pts, np.array(psc.wavelengths(len(pts))), psc.reference(name, lattice)[1][order]


def _tiled(a, n):
    reps = -(-n // len(a))
    return np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n])


def _pipeline(cam, pts, u, lam=None):
    """pupil bounds, then the splats from those bounds in place, on one stream: (bounds (n,), splats (n, m)) on the host"""
    import torch
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        P, Uu = torch.from_numpy(pts).to(dev), torch.from_numpy(u).to(dev)
        L = None if lam is None else torch.from_numpy(lam).to(dev)
        bounds = cam.pupil_bounds(P, G, None, L)
        out = cam.splat_points(P, bounds, Uu, L)
    s.synchronize()
    assert tuple(out.shape) == (len(pts), u.shape[1], 8) and out.dtype == torch.float32
    return pupil_bounds_records(bounds), splat_records(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_pupil_bounds_kernel_equals_host_twin_bitwise(gpu, name):
    cam, p = _camera(name)
    for lattice, window in CONFIGS:
        pts, lam, ok = _ordered(name, lattice)
        n = len(pts)
        # asserted on the host data: the rows the comparison is for are among the compared ones, and first
        single, full = psc.rows_of_interest(ok)
        if name == psc.STAND_IN:
            assert len(single) and single[0] == 0, lattice
        if len(full):
            assert full[0] < 5, (lattice, full)
        good = bs.valid(lam)
        assert not good[3] and good[:3].all() and good[4]          # a workgroup's four waves: three valid wavelengths and a rejected one
        for w in (None, lam):
            host = _host_bounds(cam, p, pts, lattice, window, w)
            if w is None and window is None:
                assert np.array_equal(host["count"], ok.sum(1))
            for k in PREFIXES + (n,):
                got = cam.pupil_bounds(pts[:k], lattice, window, None if w is None else w[:k])
                assert got.dtype == pupil_ref.DTYPE and got.shape == (k,)
                assert pupil_ref.same_records(got, host[:k]), (lattice, window, w is not None, k,
                                                                [(i, host[i], got[i]) for i in range(k) if host[i].tobytes() != got[i].tobytes()][:3])
            if name == mc.OUTSIDE:
                assert (host["count"] == 0).all() and (host["flags"][good if w is not None else slice(None)] == 1 << (16 + OUTSIDE_DOMAIN)).all()
            if w is not None:
                assert (host["count"][~good] == 0).all() and (host["flags"][~good] == 1 << (16 + bs.TB_WAVELENGTH)).all()
    if name in mc.LARGE_BATCH:
        pts, lam, _ = _ordered(name, 8)
        big, biglam = _tiled(pts, SLAB_PLUS_ONE), _tiled(lam, SLAB_PLUS_ONE)
        for w in (None, biglam):
            host = _tiled(_host_bounds(cam, p, pts, 8, None, None if w is None else lam), SLAB_PLUS_ONE)
            assert pupil_ref.same_records(cam.pupil_bounds(big, 8, None, w), host), w is not None
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_splat_kernel_equals_host_twin_bitwise(gpu, name):
    cam, p = _camera(name)
    pts, lam, _ = _ordered(name, G)
    n = len(pts)
    good = bs.valid(lam)
    for k, m in SPLAT_SHAPES + ((n, 7),):
        u = psc.u(k, m)
        for w in (None, lam[:k]):
            bounds, got = _pipeline(cam, pts[:k], u, w)
            assert pupil_ref.same_records(bounds, _host_bounds(cam, p, pts[:k], G, None, w)), (k, m, w is not None)
            host = _host_splats(cam, p, pts[:k], bounds, u, w)
            assert got.shape == (k, m) and splat_ref.same_records(got, host), (k, m, w is not None, splat_ref.differing(got, host))
            none = bounds["count"] == 0
            e = host[none].copy()
            assert (e["flags"] == splat_ref.NO_BOX).all()
            e["flags"] = 0
            assert not np.frombuffer(e.tobytes(), np.uint8).any()
            if k == n:
                if name not in (mc.OUTSIDE, psc.STAND_IN):
                    assert ((host["flags"] & 1) == 1).sum() >= 50 and (~none).sum() >= 20
                if w is not None:
                    assert (host["flags"][~good] == splat_ref.NO_BOX).all()
                # sx, sy and the flag word are the trace-back kernel's on the same rays
                _, o, d, empty = splat_ref.aims_and_rays(pts, bounds, u, cam.pupil_square()[0])
                if (~empty).any():
                    keep = ~empty & np.isfinite(d).all(1)        # (a NaN aim: the ray record would carry the NaN; the splat's own refusal is held above)
                    scr, fl = cam.trace_back(_records(o[keep], d[keep]), wavelengths=None if w is None else np.repeat(w, m)[keep])
                    flat = got.reshape(-1)[keep]
                    assert np.array_equal(flat["flags"], fl.astype(np.uint32))
                    assert np.array_equal(_bits(flat["sx"]), _bits(scr[:, 0])) and np.array_equal(_bits(flat["sy"]), _bits(scr[:, 1]))
    if name in mc.LARGE_BATCH:
        k, m = STRIDE_SHAPE
        big, biglam, u = _tiled(pts, k), _tiled(lam, k), psc.u(k, m)
        small = {False: _host_bounds(cam, p, pts, G), True: _host_bounds(cam, p, pts, G, None, lam)}
        for w in (None, biglam):
            bounds, got = _pipeline(cam, big, u, w)
            assert pupil_ref.same_records(bounds, _tiled(small[w is not None], k))
            host = _host_splats(cam, p, big, bounds, u, w)
            assert splat_ref.same_records(got, host), (w is not None, splat_ref.differing(got, host))
    if name == mc.OUTSIDE:      # a forced box: the trace refuses every ray for the domain's reason, the aim is written, the measures are +0
        box = np.zeros(n, _capi.PUPIL_BOUNDS_DTYPE)
        box["aim"], box["count"], box["lattice"], box["flags"] = (-0.5, -0.25, 0.5, 0.25), 7, 256, 1
        u = psc.u(n, 5)
        for w in (None, lam):
            forced = cam.splat_points(pts, box, u, w)
            assert forced.shape == (n, 5) and splat_ref.same_records(forced, _host_splats(cam, p, pts, box, u, w))
            rows = slice(None) if w is None else good
            assert (forced["flags"][rows] == OUTSIDE_DOMAIN << 8).all() and (forced["ax"] != 0).any()
            for f in ("sx", "sy", "area", "angle", "reserved"):
                assert not _bits(forced[f]).any(), f
    cam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_spectral_kernels_at_the_d_line_give_the_d_line_kernels_bits(gpu, name):
    cam, p = _camera(name)
    pts, _, _ = _ordered(name, G)
    n = len(pts)
    dline = np.full(n, bs.LAMBDA_D, F32)
    for lattice, window in CONFIGS:
        assert pupil_ref.same_records(cam.pupil_bounds(pts, lattice, window, dline), cam.pupil_bounds(pts, lattice, window)), (lattice, window)
    u = psc.u(n, 7)
    b0, s0 = _pipeline(cam, pts, u)
    b1, s1 = _pipeline(cam, pts, u, dline)
    assert pupil_ref.same_records(b0, b1) and splat_ref.same_records(s0, s1), splat_ref.differing(s0, s1)
    if name not in (mc.OUTSIDE, psc.STAND_IN):
        assert ((s0["flags"] & 1) == 1).sum() >= 50
    cam.close()


@pytest.mark.gpu
def test_out_buffers_are_reused_across_lenses(gpu):
    """One camera and one `out` buffer for the bounds and one for the splats; the lens goes from double-3 to fisheye-5 to petzval-5
    with no reallocation.  After each update every record is the new lens's (the host twin's bits): boxes that were full are all +0
    where the new lens sees nothing, their splats kSpNoBox and 32 zero bytes apart from the flag, and the sentinel row past n (n m)
    stays as it was."""
    import torch
    pts = np.ascontiguousarray(psc.points("double-3")[0][psc.device_order("double-3", G)])
    n, m = len(pts), 7
    lam, u = np.array(psc.wavelengths(n)), psc.u(n, m)
    dev = torch.device("cuda", 0)
    P, Uu, Lm = torch.from_numpy(pts).to(dev), torch.from_numpy(u).to(dev), torch.from_numpy(lam).to(dev)
    bounds = torch.full((n + 1, 12), 7.0, dtype=torch.float32, device=dev)
    splats = torch.full((n + 1, m, 8), 7.0, dtype=torch.float32, device=dev)
    cam = ZoicCamera(device=0)
    cam.set_precision(PRECISION_STRICT)
    seen = {}
    for name in ("double-3", "fisheye-5", "petzval-5"):
        lens = mc.LENSES[name]
        cam.set_abbe_numbers(None)          # (V-numbers must fit the loaded lens: cleared, and set again for the new one after its update)
        cam.set_lens_text(lens.text)
        cam.update(**mc.params(name))
        if lens.abbe is not None:
            cam.set_abbe_numbers(lens.abbe)
        for w, L in ((None, None), (lam, Lm)):
            b = cam.pupil_bounds(P, G, None, L, out=bounds[:n])
            s = cam.splat_points(P, b, Uu, L, out=splats[:n])
            torch.cuda.synchronize()
            assert b.data_ptr() == bounds.data_ptr() and s.data_ptr() == splats.data_ptr()
            assert (bounds[n] == 7.0).all().item() and (splats[n] == 7.0).all().item()
            hb = psc.host_bounds(name, G, pts=pts, lam=w)        # the host twin behind a fresh tables-only camera of the lens
            gb, gs = pupil_bounds_records(bounds[:n]), splat_records(splats[:n])
            assert pupil_ref.same_records(gb, hb), (name, w is not None)
            hs = psc.host_splats(name, pts, hb, u, w)
            assert splat_ref.same_records(gs, hs), (name, w is not None, splat_ref.differing(gs, hs))
            none = gb["count"] == 0
            assert not _bits(gb["aim"][none]).any() and not _bits(gb["screen"][none]).any() and ((gb["flags"][none] & 1) == 0).all()
            e = gs[none].copy()
            assert (e["flags"] == splat_ref.NO_BOX).all()
            e["flags"] = 0
            assert not np.frombuffer(e.tobytes(), np.uint8).any()
            if w is None:
                seen[name] = none
    # the sequence is worth its name: boxes double-3 fills are empty behind fisheye-5, and petzval-5 empties every one
    assert (~seen["double-3"]).sum() >= 40 and (seen["fisheye-5"] & ~seen["double-3"]).sum() >= 30 and seen["petzval-5"].all()
    cam.close()

"""Hero-wavelength rays (zoic_create_rays_hero_device) without a GPU: the header declares the call and its constants, the library
exports it, the Python table binds it, and the argument checks that need no device answer as the header states.

The CPU reference of the whole call (tests/hero_ref.py), checked on its own before any GPU test relies on it, for every camera of
hero_cases.CAMERAS on its standard batch: the recorded start traced with the hero's own indices gives back the oracle's hero record
(control); where the oracle accepts the same try at a companion's wavelength the reference is the oracle's own record there, where
it needs a later one the companion is lost (consistency); and what the batch exercises is pinned (census)."""
import ctypes
import os
import re

import numpy as np
import pytest

import zoic_amd
import hero_cases as hr
from library_facts import header_text
from zoic_amd import ZoicCamera, ZoicError, _capi
from zoic_amd.workloads import camera_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zoic_create_rays_hero_device"
INVALID = _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
NO_DEVICE = _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")


def _header():
    return open(os.path.join(ROOT, "include", "zoic_amd.h")).read()


def test_header_library_and_binding_table_agree():
    code = header_text()
    assert re.search(r"\bzoic_status\s+%s\s*\(" % NAME, code)
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    res, args = _capi.SYMBOLS[NAME]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                    ctypes.c_void_p, ctypes.c_void_p]
    # the threading list and the ABI history name it
    assert _header().count(NAME) >= 4


def test_constants():
    h = _header()
    assert re.search(r"#define\s+ZOIC_HERO_MAX_WAVELENGTHS\s+8\b", h)
    assert re.search(r"#define\s+ZOIC_RAY_COMPANION_LOST\s+0x100u", h)
    assert _capi.HERO_MAX_WAVELENGTHS == zoic_amd.HERO_MAX_WAVELENGTHS == 8
    assert _capi.RAY_COMPANION_LOST == zoic_amd.RAY_COMPANION_LOST == 0x100


def test_tables_only_camera_and_the_range_of_k():
    L = _capi.load()
    cam = ZoicCamera(device=-1)
    cam.update(**camera_params("C2"))
    call = lambda n, k: L.zoic_create_rays_hero_device(cam._h, n, k, None, None, None, 0, None, None)
    for k in (1, 4, 8):
        assert call(64, k) == NO_DEVICE
        assert call(0, k) == NO_DEVICE
    for k in (0, 9, 1 << 31):   # k is checked first, on every camera
        assert call(64, k) == INVALID
        assert call(0, k) == INVALID
    assert L.zoic_create_rays_hero_device(None, 64, 4, None, None, None, 0, None, None) == INVALID
    # the Python method reports the library's answer
    s = np.zeros((16, 4), np.float32)
    with pytest.raises(ZoicError) as e:
        cam.create_rays_hero(s, np.full((16, 4), 550.0, np.float32))
    assert e.value.status == NO_DEVICE
    with pytest.raises(ZoicError) as e:
        cam.create_rays_hero(s, np.full((16, 9), 550.0, np.float32))
    assert e.value.status == INVALID
    with pytest.raises(ValueError):
        cam.create_rays_hero(s, np.full(16, 550.0, np.float32))
    cam.close()


# ---- the reference alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.CAMERAS)
def test_control_the_recorded_start_reproduces_the_hero(oracle_lib, name):
    s, lam, st, words, counters, det = hr.reference(oracle_lib, name)
    live = det["planes"][6] != 0
    assert live.sum() >= 256
    ok, ends = hr.trace_starts(oracle_lib, hr.spec(name), det["starts"][live], np.ascontiguousarray(lam[live, 0]))
    assert ok.all(), int((~ok).sum())
    again = ends * np.float32(-1.0)
    hero = det["planes"][0:6, live].T
    same = (again.view(np.uint32) == np.ascontiguousarray(hero).view(np.uint32)) | (np.isnan(again) & np.isnan(hero))
    assert same.all(), int((~same.all(1)).sum())
    # ... and so does the reference's own companion at the hero's wavelength (the header's "repeats the hero's record")
    sp = hr.spec(name)
    twice = np.repeat(lam[:, :1], 2, 1)
    w2, c2 = hr.hero_reference(oracle_lib, sp.params, sp.dispersion(), s, twice, st, lens_text=sp.text)
    assert hr.same_words(w2[live, 1], w2[live, 0]).all()
    assert np.array_equal(w2[:, 0], words[:, 0]) and c2 == counters
    assert not w2[~live, 1, :7].any() and np.array_equal(w2[~live, 1, 7], w2[~live, 0, 7] | hr.LOST)


@pytest.mark.parametrize("name", hr.CAMERAS)
def test_consistency_with_the_oracle_and_census(oracle_lib, name):
    s, lam, st, words, counters, det = hr.reference(oracle_lib, name)
    planes, flags = hr.oracle_columns(oracle_lib, hr.spec(name), s, lam, st)
    own = np.concatenate([planes.view(np.uint32), flags[None]], 0).transpose(1, 2, 0)      # (n, k, 8): the oracle's ray at each wavelength
    assert np.array_equal(own[:, 0], words[:, 0])                                              # NaN-free inputs: plain equality
    tries = ((flags >> 1) & 31).astype(np.int32)
    live = det["planes"][6] != 0
    same = live[:, None] & (tries == tries[:, :1])
    later = live[:, None] & (tries > tries[:, :1])
    assert hr.same_words(words[same], own[same]).all(), int((~hr.same_words(words[same], own[same])).sum())
    assert not words[later][:, :7].any() and np.array_equal(words[later][:, 7], np.broadcast_to(words[:, :1, 7], later.shape)[later] | hr.LOST)
    # the counters are column 0's: the oracle's own, run on that column without the start recording
    from fuzz_cameras import _oracle_spectral
    sp = hr.spec(name)
    own0, c0 = _oracle_spectral(oracle_lib, sp.params, sp.dispersion(), s, np.ascontiguousarray(lam[:, 0]), st, lens_text=sp.text)
    assert counters == c0 and (c0["succesRays"], c0["vignettedRays"]) == (int(live.sum()), int((~live).sum()))
    assert np.array_equal(own0["planes"].view(np.uint32), det["planes"].view(np.uint32)) and np.array_equal(own0["flags"], det["flags"])
    got = hr.census(words, tries)
    print(name, got)
    assert got == hr.CENSUS[name], (name, got)
    for family, count in got.items():
        assert count >= hr.FAMILY_MIN or (name, family) in hr.THIN, (name, family, count)
    for (cam, family), why in hr.THIN.items():    # a family the camera cannot produce: none at all
        assert hr.CENSUS[cam][family] == 0 and why


def test_reference_rejections_and_the_thin_lens(oracle_lib):
    """the reference's own bookkeeping on a small batch: an invalid hero rejects its row and counts nowhere, an invalid companion is
    rejected alone, and the thin lens copies the hero into every valid column"""
    sp = hr.spec("C2")
    s, lam, st = hr.inputs(256, 4)
    lam = lam.copy()
    lam[3, 0], lam[5, 2], lam[7, 1:] = np.nan, 830.1, 0.0
    base, cb = hr.hero_reference(oracle_lib, sp.params, sp.dispersion(), np.delete(s, 3, 0), np.delete(hr.inputs(256, 4)[1], 3, 0), np.delete(st, 3, 0))
    w, c = hr.hero_reference(oracle_lib, sp.params, sp.dispersion(), s, lam, st)
    assert c == cb
    assert not w[3, :, :7].any() and (w[3, :, 7] == hr.REJECTED).all()
    hit = np.zeros((256, 4), bool)
    hit[5, 2] = hit[7, 1:] = True
    assert not w[hit][:, :7].any() and (w[hit][:, 7] == hr.REJECTED).all()
    keep = np.delete(~hit, 3, 0)
    assert np.array_equal(np.delete(w, 3, 0)[keep], base[keep])
    thin = dict(camera_params("C1"), opticalVignettingDistance=5.0)
    t, _ = hr.hero_reference(oracle_lib, thin, None, s, lam, st)
    ok = hr.valid(lam)
    for j in range(1, 4):
        rows = ok[:, 0] & ok[:, j]
        assert np.array_equal(t[rows, j], t[rows, 0])
    assert (t[~(ok[:, :1] & ok)][:, 7] == hr.REJECTED).all() and not t[~(ok[:, :1] & ok)][:, :7].any()

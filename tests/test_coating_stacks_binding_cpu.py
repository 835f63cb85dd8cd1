"""Multilayer coatings without a GPU, the interface: the C-ABI declares, exports and binds zoic_camera_set_coating_stacks and
zoic_camera_get_coating_stacks; on a tables-only camera the setter refuses what include/zoic_amd.h says it refuses and a refused call
changes nothing; order, default, clear and update behave as test_transmittance_cpu.py shows for the single film."""
import ctypes
import re

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera, ZoicError

from coating_stack_ref import MAX_LAYERS, Q, QHQ, R8, f32_pairs
from differentials_spectral_ref import tables
from library_facts import header_text

NAMES = ("zoic_camera_set_coating_stacks", "zoic_camera_get_coating_stacks")
F32 = np.float32
INVALID = _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")


def test_abi_declares_exports_and_binds_the_calls():
    text = header_text()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS and hasattr(raw, name) and hasattr(_capi.load(), name), name
        assert len(_capi.SYMBOLS[name][1]) == 5
    assert re.search(r"#define\s+ZOIC_COATING_MAX_LAYERS\s+8\b", text) and _capi.COATING_MAX_LAYERS == MAX_LAYERS == 8
    assert _capi.load().zoic_abi_version() == 5 and _capi.ABI_VERSION == 5
    assert callable(ZoicCamera.set_coating_stacks) and callable(ZoicCamera.coating_stacks)
    for method in ("transmittance", "create_ghost_rays", "trace_back_transmittance", "splat_transmittance", "set_coatings"):
        assert "set_coating_stacks" in getattr(ZoicCamera, method).__doc__, method


def _arrays(count, stack=Q):
    layers = np.full(count, len(stack), np.int32)
    index, thick = np.zeros((count, MAX_LAYERS), F32), np.zeros((count, MAX_LAYERS), F32)
    index[:, :len(stack)], thick[:, :len(stack)] = [p[0] for p in stack], [p[1] for p in stack]
    return layers, index, thick


def test_errors_on_a_tables_only_camera():
    lib = _capi.load()
    p, info = tables("C2")[:2]
    cam = ZoicCamera(device=-1)
    cam.update(**p)
    count = info["lensCount"]
    s, g = lib.zoic_camera_set_coating_stacks, lib.zoic_camera_get_coating_stacks
    P = lambda a: a.ctypes.data  # noqa: E731
    L, I, D = _arrays(count)
    assert s(None, count, P(L), P(I), P(D)) == INVALID
    assert s(cam._h, count, None, P(I), P(D)) == INVALID and s(cam._h, count, P(L), None, P(D)) == INVALID
    assert s(cam._h, count, P(L), P(I), None) == INVALID
    L1, I1, D1 = _arrays(count + 1)
    assert s(cam._h, count + 1, P(L1), P(I1), P(D1)) == INVALID               # not the lens's surface count
    L33, I33, D33 = _arrays(33)
    assert s(cam._h, -1, P(L), P(I), P(D)) == INVALID and s(cam._h, 33, P(L33), P(I33), P(D33)) == INVALID
    for bad in (-1, 9):
        a = L.copy()
        a[3] = bad
        assert s(cam._h, count, P(a), P(I), P(D)) == INVALID, bad
    for bad_n, bad_d in ((0.5, 100.0), (4.5, 100.0), (np.nan, 100.0), (np.inf, 100.0), (-1.38, 100.0), (0.0, 100.0), (1.38, 0.0),
                         (1.38, -5.0), (1.38, 1000.5), (1.38, np.nan), (1.38, np.inf)):
        a, b = I.copy(), D.copy()
        a[3, 0], b[3, 0] = bad_n, bad_d
        assert s(cam._h, count, P(L), P(a), P(b)) == INVALID, (bad_n, bad_d)
    assert not cam.coating_stacks()["layers"].any()                            # nothing was taken from the refused calls
    a, b = I.copy(), D.copy()
    a[:, 1:], b[:, 1:] = np.nan, -1.0                                          # entries past layers[i] are not looked at
    assert s(cam._h, count, P(L), P(a), P(b)) == 0
    got = cam.coating_stacks()
    assert (got["layers"] == 1).all() and not got["index"][:, 1:].any() and not got["thickness_nm"][:, 1:].any()
    edge = _arrays(count, [(1.0, 1000.0), (4.0, 1e-3)])                        # the limits themselves are taken
    assert s(cam._h, count, *[P(x) for x in edge]) == 0
    # a refused call leaves the table in force as it was
    before = cam.coating_stacks()
    bad = L.copy()
    bad[0] = 9
    assert s(cam._h, count, P(bad), P(I), P(D)) == INVALID
    after = cam.coating_stacks()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert g(None, 0, None, None, None) == -1 and g(cam._h, -1, None, None, None) == -1
    assert g(cam._h, 0, None, None, None) == count
    assert s(cam._h, 0, None, None, None) == 0 and not cam.coating_stacks()["layers"].any()
    cam.close()


def test_order_default_clear_and_update():
    """coating_stacks(): trace order = reversed file order, and each interface's layers reversed (file: layer 0 at the front-side medium;
    table: as a forward ray, rear to front, meets them); the default is no stack anywhere; the override survives an update of the same
    lens and fails one whose lens has another surface count"""
    p, info = tables("C2")[:2]
    count = info["lensCount"]
    cam = ZoicCamera(device=-1)
    empty = cam.coating_stacks()
    assert empty["layers"].shape == (0,) and empty["index"].shape == (0, 8) and empty["thickness_nm"].shape == (0, 8)   # no lens yet
    stacks = [QHQ, None, R8, [], Q] + [QHQ] * (count - 5)
    cam.set_coating_stacks(stacks)                                             # before the first update: any count is taken
    cam.update(**p)
    got = cam.coating_stacks()
    assert got["layers"].dtype == np.int32 and got["index"].dtype == F32 and got["index"].shape == (count, 8)
    assert got["layers"].tolist() == [len(s or []) for s in stacks][::-1]
    for i, s in enumerate(stacks[::-1]):
        want = np.array(f32_pairs(s or [])[::-1], F32).reshape(-1, 2)
        assert np.array_equal(got["index"][i, :len(want)], want[:, 0]) and np.array_equal(got["thickness_nm"][i, :len(want)], want[:, 1]), i
        assert not got["index"][i, len(want):].any() and not got["thickness_nm"][i, len(want):].any()
    cam.update(**dict(p, fStop=8.0))
    assert np.array_equal(cam.coating_stacks()["layers"], got["layers"])
    p3 = tables("C3")[0]
    count3 = tables("C3")[1]["lensCount"]
    assert count3 != count
    with pytest.raises(ZoicError) as e:
        cam.update(**p3)
    assert e.value.status == INVALID and "zoic_camera_set_coating_stacks" in str(e.value)
    cam.set_coating_stacks(None)
    cam.update(**p3)
    assert not cam.coating_stacks()["layers"].any() and len(cam.coating_stacks()["layers"]) == count3
    with pytest.raises(ZoicError):
        cam.set_coating_stacks(stacks)                                         # a loaded lens: the count must be its own
    with pytest.raises(ValueError):
        cam.set_coating_stacks([[(1.38, 100.0)] * 9] + [None] * (count3 - 1))  # more layers than a row holds
    cam.set_coating_stacks([Q] * count3)
    assert (cam.coating_stacks()["layers"] == 1).all()
    cam.set_coating_stacks([None] * count3)                                    # layers all 0: a table, but no stack
    assert not cam.coating_stacks()["layers"].any()
    cam.close()
    wrong = ZoicCamera(device=-1)
    wrong.set_coating_stacks(stacks[:3])
    with pytest.raises(ZoicError):
        wrong.update(**p)
    wrong.close()


def test_a_stack_leaves_the_film_table_alone():
    p, info = tables("C2")[:2]
    count = info["lensCount"]
    cam = ZoicCamera(device=-1)
    cam.update(**p)
    cam.set_coatings(np.full(count, 1.38, F32), 550.0)
    films = cam.coatings()
    cam.set_coating_stacks([QHQ] * count)
    assert all(np.array_equal(films[k], cam.coatings()[k]) for k in films)
    cam.set_coatings(None, None)
    assert (cam.coating_stacks()["layers"] == 3).all()
    cam.close()

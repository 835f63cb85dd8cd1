"""Hero-wavelength rays (zoic_create_rays_hero_device) without a GPU: the header declares the call and its constants, the library
exports it, the Python table binds it, and the argument checks that need no device answer as the header states."""
import ctypes
import os
import re

import numpy as np
import pytest

import zoic_amd
from zoic_amd import ZoicCamera, ZoicError, _capi
from zoic_amd.workloads import camera_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zoic_create_rays_hero_device"
INVALID = _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
NO_DEVICE = _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")


def _header():
    return open(os.path.join(ROOT, "include", "zoic_amd.h")).read()


def test_header_library_and_binding_table_agree():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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

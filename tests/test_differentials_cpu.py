"""Traced ray differentials without a GPU: the C-ABI declares and exports them, the transfer math of csrc/differentials.hpp
(compiled for the host) agrees with finite differences of a numpy restatement of the trace, and the gfx950 kernels stay within
their register budget."""
import ctypes
import re

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera
from zoic_amd.workloads import camera_params

import host_drivers
from differentials_ref import kolb_jacobian_fd, passing_rays, rel_err, surfaces, trace
from library_facts import header_text, kernel_resources

NEW = ("zoic_ray_differentials_device", "zoic_create_rays_arnold_differentials")


def test_abi_declares_and_exports_differentials():
    text = header_text()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
    assert "zoic_ray_differential;" in text
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(_capi.RayDifferential) == 48
    assert _capi.load().zoic_abi_version() == 5


@pytest.fixture(scope="module")
def driver():
    return host_drivers.differentials()


@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_tangents_match_finite_differences(cfg, driver, oracle_lib):
    """On ~10 k random passing rays per lens: the host-compiled tangent trace agrees with f64 central differences of the numpy
    restatement (L held fixed); the restatement is first checked against the oracle's own trace."""
    p = camera_params(cfg)
    p["useImage"] = False   # the interfaces are all this test needs
    p.pop("bokehPath", None)
    cam = ZoicCamera(device=-1)   # ZOIC_DEVICE_NONE: the host precompute only
    cam.update(**p)
    info = cam.info()
    cam.close()
    oc = oracle_lib.OracleCamera()
    oc.update(**p)
    lt = oc.lens_table()
    assert np.array_equal(lt["elements"], info["elements"][:lt["lensCount"]])
    surf = surfaces(info)
    hs = np.float32(np.float32(p["sensorWidth"]) * np.float32(0.5))
    o, d, ref_o, ref_d = passing_rays(oc, info, hs, np.random.RandomState(11), 10000)
    n = len(o)
    assert n >= 5000, "%s: only %d passing rays" % (cfg, n)
    # the restatement is the oracle's trace
    ro, rd = trace(surf, o, d)
    eo = np.linalg.norm(ro - ref_o, axis=1) / np.linalg.norm(ref_o, axis=1)
    ed = np.linalg.norm(rd - ref_d, axis=1) / np.linalg.norm(ref_d, axis=1)
    assert np.median(eo) < 1e-6 and np.median(ed) < 1e-6, (cfg, np.median(eo), np.median(ed))
    # (the f32 oracle's hit points carry its own rounding -- e.g. the stop, traced as a sphere of |R| ~ 1e4 cm: origins to 1e-4 at the tail)
    assert np.percentile(eo, 99.9) <= 1e-4 and np.percentile(ed, 99.9) <= 1e-5, (cfg, eo.max(), ed.max())
    # the tangents
    out = np.zeros((n, 12), np.float32)
    prim = np.zeros((n, 6), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    c = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(fp)  # noqa: E731
    sf = np.ascontiguousarray(surf, np.float32)
    o32, d32 = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    driver.zd_trace(len(surf), c(sf), ctypes.c_float(hs), n, c(o32), c(d32), out.ctypes.data_as(fp), prim.ctypes.data_as(fp))
    assert np.allclose(prim[:, 0:3], -ref_o, rtol=1e-4, atol=1e-4)   # the driver's primal is the same ray (after the flip)
    fd = kolb_jacobian_fd(surf, hs, o, d)
    e = rel_err(out, fd)
    assert np.isfinite(out).all()
    assert np.median(e) <= 1e-5 and np.percentile(e, 99.9) <= 1e-3, (cfg, float(np.median(e)), float(np.percentile(e, 99.9)))


def test_differential_kernels_budget():
    """0 scratch, 0 VGPR spills, <= 128 VGPRs for every differential kernel of the built library (its code object's metadata)."""
    res = {k: v for k, v in kernel_resources().items() if "differentials_kernel" in k}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["vgpr"] + v["agpr"] <= 128, (k, v)

"""Traced ray differentials without a GPU: the C-ABI declares and exports them, the transfer math of csrc/differentials.hpp
(compiled for the host) agrees with finite differences of a numpy restatement of the trace, and the gfx950 kernels stay within
their register budget."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from zoic_amd import _capi
from zoic_amd.camera import ZoicCamera
from zoic_amd.workloads import camera_params

from differentials_ref import kolb_jacobian_fd, rel_err, surfaces, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zoic_amd", "csrc")
NEW = ("zoic_ray_differentials_device", "zoic_create_rays_arnold_differentials")


def test_abi_declares_and_exports_differentials():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zoic_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS, name
    assert "zoic_ray_differential;" in text
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(_capi.RayDifferential) == 48
    assert _capi.load().zoic_abi_version() == 5


DRIVER = r"""
#include "differentials.hpp"
extern "C" int zd_trace(int count, const float *surf, float halfSensor, int n, const float *o, const float *d, float *out, float *prim)
{
    zoic::Surface S[zoic::kMaxSurfaces] = {};
    for (int i = 0; i < count; ++i) { S[i].center = surf[4 * i]; S[i].radius2 = surf[4 * i + 1]; S[i].sign = surf[4 * i + 2]; S[i].eta = surf[4 * i + 3]; }
    for (int r = 0; r < n; ++r) {
        zoic::V3 po, pd;
        const zoic::RayDifferential g = zoic::kolb_differentials([&](int i) { return S[i]; }, count, halfSensor,
                                                                  zoic::V3{o[3 * r], o[3 * r + 1], o[3 * r + 2]},
                                                                  zoic::V3{d[3 * r], d[3 * r + 1], d[3 * r + 2]}, &po, &pd);
        const zoic::V3 v[6] = {g.dOdx, g.dOdy, g.dDdx, g.dDdy, po, pd};
        for (int k = 0; k < 4; ++k) { out[12 * r + 3 * k] = v[k].x; out[12 * r + 3 * k + 1] = v[k].y; out[12 * r + 3 * k + 2] = v[k].z; }
        for (int k = 0; k < 2; ++k) { prim[6 * r + 3 * k] = v[4 + k].x; prim[6 * r + 3 * k + 1] = v[4 + k].y; prim[6 * r + 3 * k + 2] = v[4 + k].z; }
    }
    return 0;
}
"""


def _clangxx():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no clang++ to build the host driver of csrc/differentials.hpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("diffdriver")
    src, so = d / "driver.cpp", d / "driver.so"
    src.write_text(DRIVER)
    subprocess.check_call([_clangxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))


def _passing_rays(oc, info, hs, rs, want):
    """random sensor points aimed at random points of the rear element; the ones the oracle's trace lets through"""
    import oracle
    L = oracle.lib()
    el = info["elements"]
    n = want * 40
    o = np.stack([rs.uniform(-1, 1, n) * hs, rs.uniform(-0.7, 0.7, n) * hs, np.full(n, info["originShift"])], 1).astype(np.float32)
    r = np.sqrt(rs.uniform(0, 1, n)) * el[0, 3] * 0.5
    a = rs.uniform(0, 2 * np.pi, n)
    d = np.stack([r * np.cos(a) - o[:, 0], r * np.sin(a) - o[:, 1], np.full(n, -el[0, 1])], 1).astype(np.float32)
    keep, po, pd = [], [], []
    hits = (oracle.V3 * 128)()
    nh = ctypes.c_int()
    for i in range(n):
        oo, dd = oracle.V3(*o[i]), oracle.V3(*d[i])
        if L.zo_trace_record(oc._h, ctypes.byref(oo), ctypes.byref(dd), hits, ctypes.byref(nh)):
            keep.append(i); po.append((oo.x, oo.y, oo.z)); pd.append((dd.x, dd.y, dd.z))
            if len(keep) == want:
                break
    return o[keep], d[keep], np.array(po, np.float64), np.array(pd, np.float64)


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
    o, d, ref_o, ref_d = _passing_rays(oc, info, hs, np.random.RandomState(11), 10000)
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import code_object_regs
    finally:
        sys.path.pop(0)
    res = {k: v for k, v in code_object_regs.kernel_resources(_capi.LIB_PATH).items() if "differentials_kernel" in k}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["vgpr"] + v["agpr"] <= 128, (k, v)

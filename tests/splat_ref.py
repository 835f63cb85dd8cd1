"""An independent restatement of the lens splats (zoic_amd/csrc/splat.hpp), written from the definition: the aims and the rays come
from zoic_amd.pupil_rays, each ray is traced by code that is already pinned -- the library's host call zoic_trace_back_ray_jacobian, or
its _spectral form, on a tables-only camera (held against f64 central differences by tests/test_traceback_jacobian_cpu.py) -- and the
two measures are computed by numpy float32 operations in the header's order, each one correctly rounded operation.  Records of empty
boxes are built by the rule.  A helper, not a test."""
import ctypes

import numpy as np

from zoic_amd import _capi, pupil_bounds_records, pupil_rays

F32 = np.float32
DTYPE = np.dtype(_capi.SPLAT_DTYPE)
NO_BOX = 1 << 12
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(F32)[0]


def number(v):
    """tbj_number: a NaN becomes the one quiet NaN"""
    v = np.asarray(v, F32).copy()
    v[np.isnan(v)] = QUIET_NAN
    return v


def aims_and_rays(points, bounds, u, z):
    """(aims (n m, 2), origins (n m, 3), dirs (n m, 3), empty (n m,)) float32, point-major, for points (n,3), their records (n,) and
    u (n,m,2).  pupil_rays gives dirs = points - aims; from the origin its dirs are 0 - aims, so aims = 0 - (0 - aims): two exact
    operations (an aim is never -0: a box side is a sum or a difference of finite numbers, or a clamp to one)."""
    b = pupil_bounds_records(bounds)
    u = np.ascontiguousarray(u, F32)
    n, m = u.shape[0], u.shape[1]
    pts = np.repeat(np.ascontiguousarray(points, F32).reshape(-1, 3), m, axis=0)
    bb = np.repeat(b, m)
    uu = u.reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        o, d, _ = pupil_rays(pts, bb, uu, z)
        _, neg, _ = pupil_rays(np.zeros_like(pts), bb, uu, z)
        aims = (F32(0.0) - neg)[:, 0:2]
    empty = (bb["count"] == 0) | ((bb["flags"] & 1) == 0)
    assert len(o) == n * m
    return aims, o, d, empty


def trace_jacobian(cam, o, d, lam=None):
    """zoic_trace_back_ray_jacobian (lam None) or its _spectral form on every ray: (ps (k,2) float32, flags (k,) uint32, J (k,12))"""
    lib, h = _capi.load(), cam._h
    k = len(o)
    ps, fl, J = np.zeros((k, 2), F32), np.zeros(k, np.uint32), np.zeros((k, 12), F32)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    V, FP, UP = ctypes.POINTER(_capi.Vec3), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    po, pd, pp, pf, pj = o.ctypes.data, d.ctypes.data, ps.ctypes.data, fl.ctypes.data, J.ctypes.data
    lam = None if lam is None else np.broadcast_to(np.asarray(lam, F32), (k,))
    for i in range(k):
        a = (ctypes.cast(po + 12 * i, V), ctypes.cast(pd + 12 * i, V))
        t = (ctypes.cast(pp + 8 * i, FP), ctypes.cast(pf + 4 * i, UP), ctypes.cast(pj + 48 * i, FP))
        rc = lib.zoic_trace_back_ray_jacobian(h, *a, *t) if lam is None else lib.zoic_trace_back_ray_jacobian_spectral(h, *a, float(lam[i]), *t)
        assert rc == 0, rc
    return ps, fl, J


def measures(J, d):
    """(area, angle) float32 of traced rays in the header's order: area = J3 J10 - J4 J9; angle = (area (r2 r)) / dz with
    r2 = (dx dx + dy dy) + dz dz, r = sqrt(r2).  numpy's float32 product, sum, difference, root and quotient are each correctly rounded."""
    J, d = np.asarray(J, F32), np.asarray(d, F32)
    with np.errstate(all="ignore"):
        p0 = J[:, 3] * J[:, 10]
        p1 = J[:, 4] * J[:, 9]
        area = p0 - p1
        xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
        r2 = (xx + yy) + zz
        r = np.sqrt(r2)
        r3 = r2 * r
        num = area * r3
        angle = num / d[:, 2]
    assert area.dtype == angle.dtype == F32
    return area, angle


def reference(cam, points, bounds, u, lam=None):
    """the (n, m) records of points (n,3), their pupil-bounds records and u (n,m,2); lam: None (d-line) or (n,) wavelengths (nm).
    Also returns (dirs (n m, 3), J (n m, 12)) of the rays, zero rows for the empty boxes."""
    u = np.ascontiguousarray(u, F32)
    n, m = u.shape[0], u.shape[1]
    z = cam.pupil_square()[0]
    aims, o, d, empty = aims_and_rays(points, bounds, u, z)
    go = np.flatnonzero(~empty)
    ps, fl, J = np.zeros((n * m, 2), F32), np.zeros(n * m, np.uint32), np.zeros((n * m, 12), F32)
    ps[go], fl[go], J[go] = trace_jacobian(cam, o[go], d[go], None if lam is None else np.repeat(np.asarray(lam, F32), m)[go])
    out = np.zeros(n * m, DTYPE)
    out["flags"] = np.where(empty, np.uint32(NO_BOX), fl)
    out["sx"], out["sy"] = ps[:, 0], ps[:, 1]
    out["ax"] = np.where(empty, F32(0.0), number(aims[:, 0]))
    out["ay"] = np.where(empty, F32(0.0), number(aims[:, 1]))
    traced = ~empty & ((fl & 1) == 1)
    area, angle = measures(J, d)
    out["area"] = np.where(traced, number(area), F32(0.0))
    out["angle"] = np.where(traced, number(angle), F32(0.0))
    d = np.where(empty[:, None], F32(0.0), d)
    return out.reshape(n, m), d, J


def same_records(a, b):
    """bit for bit, all 32 bytes of every record (floats compared as their bits)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(a, b):
    """the flat indices of the records that differ, for an assertion's message"""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return [(i, a[i], b[i]) for i in range(min(len(a), len(b))) if a[i].tobytes() != b[i].tobytes()][:4]

"""Host builds of the csrc/*.hpp arithmetic for the tests: the one clang++ lookup, the one compile line, the seven driver sources and
their ctypes wrappers.  Each source is compiled at most once per process; every later request gets the same loaded library.  A helper,
not a test."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from device_cases import bits_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zoic_amd", "csrc")
F32 = np.float32


def clangxx():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no clang++ to build the host drivers of csrc/*.hpp")


_LIBS = {}


def _build(key, source):
    """the loaded host build of `source`, compiled on the first request for `key` (the directory goes once the library is mapped).
    -Bsymbolic: the library itself is loaded RTLD_GLOBAL (zoic_amd/_capi.py) and exports the headers' inline functions as weak symbols
    (zoic::splat_point, zoic::trace_back_ray, ...); without it every call of a driver that the compiler did not inline binds to the
    LIBRARY's copy, and the "host twin" is the library's own object code whatever the header under csrc/ says."""
    if key not in _LIBS:
        with tempfile.TemporaryDirectory(prefix="zoic_%s_driver_" % key) as d:
            src, so = os.path.join(d, "driver.cpp"), os.path.join(d, "driver.so")
            with open(src, "w") as f:
                f.write(source)
            subprocess.check_call([clangxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-I" + CSRC,
                                   "-I" + os.path.join(ROOT, "include"), src, "-o", so])
            _LIBS[key] = ctypes.CDLL(so)
    return _LIBS[key]


# ---- csrc/differentials.hpp -----------------------------------------------------------------------------------------------------
DIFFERENTIALS = r"""
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


def differentials():
    """zd_trace"""
    return _build("differentials", DIFFERENTIALS)


# ---- csrc/spectral.hpp ----------------------------------------------------------------------------------------------------------
SPECTRAL = r"""
#include "spectral.hpp"
extern "C" int zs_terms(int count, const float *iorD, const float *b, int n, const float *lambda, float *ior1, float *ior2, float *eta,
                        int *tir, int *valid)
{
    zoic::SpectralTable W{};
    W.count = count;
    for (int i = 0; i < count; ++i) { W.iorD[i] = iorD[i]; W.cauchyB[i] = b[i]; }
    for (int r = 0; r < n; ++r) {
        valid[r] = zoic::spectral_valid(lambda[r]) ? 1 : 0;
        const float dl = zoic::spectral_dl(lambda[r]);
        for (int i = 0; i < count; ++i) {
            float a, c;
            zoic::spectral_iors(&W, count, i, dl, a, c);
            ior1[r * count + i] = a; ior2[r * count + i] = c;
            eta[r * count + i] = zoic::spectral_eta(a, c);
            tir[r * count + i] = zoic::spectral_tir_possible(a, c) ? 1 : 0;
        }
    }
    return 0;
}
"""


def spectral():
    """zs_terms"""
    return _build("spectral", SPECTRAL)


# ---- csrc/differentials_spectral.hpp --------------------------------------------------------------------------------------------
DIFFERENTIALS_SPECTRAL = r"""
#include "differentials_spectral.hpp"
// surf: count x (center, radius2, sign, eta_d); disp: count x (iorD, cauchyB); lambda: one per ray.  out 12, chroma 6, prim 6 floats
// per ray.  mode 0: kolb_differentials on the d-line table; 1: spectral, screen tangents only; 2: with the wavelength tangent
extern "C" int zds_trace(int mode, int count, const float *surf, const float *disp, float halfSensor, int n, const float *lambda,
                         const float *o, const float *d, float *out, float *chroma, float *prim)
{
    using namespace zoic;
    Surface S[kMaxSurfaces] = {};
    SpectralTable W = {};
    W.count = count;
    for (int i = 0; i < count; ++i) {
        S[i].center = surf[4 * i]; S[i].radius2 = surf[4 * i + 1]; S[i].sign = surf[4 * i + 2]; S[i].eta = surf[4 * i + 3];
        W.iorD[i] = disp[2 * i]; W.cauchyB[i] = disp[2 * i + 1];
    }
    const auto surfAt = [&](int i) { return S[i]; };
    const SpectralTable *WP = &W;
    for (int r = 0; r < n; ++r) {
        const V3 o0{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, d0{d[3 * r], d[3 * r + 1], d[3 * r + 2]};
        V3 po, pd;
        SpectralDifferential g{};
        if (mode == 0) g.screen = kolb_differentials(surfAt, count, halfSensor, o0, d0, &po, &pd);
        else if (mode == 1) g = kolb_differentials_spectral<false>(surfAt, WP, count, lambda[r], halfSensor, o0, d0, &po, &pd);
        else g = kolb_differentials_spectral<true>(surfAt, WP, count, lambda[r], halfSensor, o0, d0, &po, &pd);
        const V3 v[8] = {g.screen.dOdx, g.screen.dOdy, g.screen.dDdx, g.screen.dDdy, g.dOdl, g.dDdl, po, pd};
        for (int k = 0; k < 4; ++k) { out[12 * r + 3 * k] = v[k].x; out[12 * r + 3 * k + 1] = v[k].y; out[12 * r + 3 * k + 2] = v[k].z; }
        for (int k = 0; k < 2; ++k) { chroma[6 * r + 3 * k] = v[4 + k].x; chroma[6 * r + 3 * k + 1] = v[4 + k].y; chroma[6 * r + 3 * k + 2] = v[4 + k].z; }
        for (int k = 0; k < 2; ++k) { prim[6 * r + 3 * k] = v[6 + k].x; prim[6 * r + 3 * k + 1] = v[6 + k].y; prim[6 * r + 3 * k + 2] = v[6 + k].z; }
    }
    return 0;
}
"""


def differentials_spectral():
    """zds_trace, called through run_differentials_spectral"""
    return _build("differentials_spectral", DIFFERENTIALS_SPECTRAL)


def run_differentials_spectral(drv, mode, surf, disp, hs, lam, o, d):
    """(out (n,12), chroma (n,6), prim (n,6)) float32 of the host driver"""
    n = len(o)
    out, chroma, prim = np.zeros((n, 12), F32), np.zeros((n, 6), F32), np.zeros((n, 6), F32)
    fp = ctypes.POINTER(ctypes.c_float)
    keep = [np.ascontiguousarray(a, F32) for a in (surf, np.stack([disp["ior_d"], disp["cauchy_b"]], 1), lam, o, d)]
    c = [a.ctypes.data_as(fp) for a in keep]
    rc = drv.zds_trace(int(mode), len(surf), c[0], c[1], ctypes.c_float(float(hs)), n, c[2], c[3], c[4], out.ctypes.data_as(fp),
                       chroma.ctypes.data_as(fp), prim.ctypes.data_as(fp))
    assert rc == 0
    return out, chroma, prim


# ---- csrc/transmittance.hpp -----------------------------------------------------------------------------------------------------
TRANSMITTANCE = r"""
#include "transmittance.hpp"
// surf: count x (center, radius2, sign, housing2); disp: count x (iorD, cauchyB); film: count x (index, lambda0); lambda: one per ray
extern "C" int ztr_trace(int count, const float *surf, const float *disp, const float *film, int n, const float *lambda, const float *o,
                         const float *d, float *T)
{
    using namespace zoic;
    Surface S[kMaxSurfaces] = {};
    SpectralTable W = {};
    FilmTable F = {};
    W.count = F.count = count;
    for (int i = 0; i < count; ++i) {
        S[i].center = surf[4 * i]; S[i].radius2 = surf[4 * i + 1]; S[i].sign = surf[4 * i + 2]; S[i].housing2 = surf[4 * i + 3];
        W.iorD[i] = disp[2 * i]; W.cauchyB[i] = disp[2 * i + 1];
        F.index[i] = film[2 * i]; F.lambda0[i] = film[2 * i + 1];
    }
    const Surface *SP = S;
    const SpectralTable *WP = &W;
    const FilmTable *FP = &F;
    for (int r = 0; r < n; ++r)
        T[r] = path_transmittance(SP, WP, FP, count, lambda[r], V3{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, V3{d[3 * r], d[3 * r + 1], d[3 * r + 2]});
    return 0;
}
extern "C" void ztr_cospi(int n, const float *x, float *y) { for (int i = 0; i < n; ++i) y[i] = zoic::film_cospi(x[i]); }
extern "C" float ztr_interface(float n1, float n2, float ci, float ct, float nc, float lambda0, float lambda)
{
    return zoic::interface_transmittance(n1, n2, ci, ct, nc, lambda0, lambda);
}
"""


def transmittance():
    """ztr_trace (called through run_transmittance), ztr_cospi, ztr_interface"""
    drv = _build("transmittance", TRANSMITTANCE)
    drv.ztr_interface.restype = ctypes.c_float
    drv.ztr_interface.argtypes = [ctypes.c_float] * 7
    return drv


def run_transmittance(drv, surf, disp, lam, o, d, film=None, housing2=None):
    """(n,) float32 T of the host driver; surf = dref.surfaces(info); film = (index, lambda0) in trace order; housing2 None: no clip"""
    n, count = len(o), len(surf)
    h2 = np.full(count, np.inf, F32) if housing2 is None else np.asarray(housing2, F32)
    s4 = np.stack([surf[:, 0], surf[:, 1], surf[:, 2], h2], 1)
    fl = np.zeros((count, 2), F32) if film is None else np.stack([film[0], film[1]], 1)
    keep = [np.ascontiguousarray(a, F32) for a in (s4, np.stack([disp["ior_d"], disp["cauchy_b"]], 1), fl, lam, o, d)]
    fp = ctypes.POINTER(ctypes.c_float)
    c = [a.ctypes.data_as(fp) for a in keep]
    T = np.full(n, -1.0, F32)
    assert drv.ztr_trace(count, c[0], c[1], c[2], n, c[3], c[4], c[5], T.ctypes.data_as(fp)) == 0
    return T


# ---- csrc/ghost.hpp -------------------------------------------------------------------------------------------------------------
GHOST = r"""
#include "ghost.hpp"
using namespace zoic;
// rows: count x (radius, thickness, aperture); media: count x (iorD, cauchyB, filmIndex, filmLambda0)
static void tables(int model, int count, const float *rows, int stop, float user, const float *media, GhostTable &G, GhostMedia &M)
{
    float radius[kMaxSurfaces] = {}, thickness[kMaxSurfaces] = {}, aperture[kMaxSurfaces] = {};
    M = GhostMedia{};
    for (int i = 0; i < count && i < kMaxSurfaces; ++i) {
        radius[i] = rows[3 * i]; thickness[i] = rows[3 * i + 1]; aperture[i] = rows[3 * i + 2];
        M.iorD[i] = media[4 * i]; M.cauchyB[i] = media[4 * i + 1]; M.filmIndex[i] = media[4 * i + 2]; M.filmLambda0[i] = media[4 * i + 3];
    }
    fill_ghost_table(G, model, count, radius, thickness, aperture, stop, user);
}
static void put(float *out, const GhostRay &g)
{
    out[0] = g.ox; out[1] = g.oy; out[2] = g.oz; out[3] = g.dx; out[4] = g.dy; out[5] = g.dz; out[6] = g.weight;
    __builtin_memcpy(out + 7, &g.flags, 4);
}
// ghost_trace of one pair (a = b = -1: the plain path) from n starts; out: n x 8
extern "C" int zgh_trace(int model, int count, const float *rows, int stop, float user, const float *media, int a, int b, int n,
                         const float *lambda, const float *o, const float *d, float *out)
{
    GhostTable G; GhostMedia M;
    tables(model, count, rows, stop, user, media, G, M);
    const GhostTable *GP = &G; const GhostMedia *MP = &M;
    for (int r = 0; r < n; ++r)
        put(out + 8 * r, ghost_trace(GP, MP, a, b, lambda[r], V3{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, V3{d[3 * r], d[3 * r + 1], d[3 * r + 2]}));
    return G.model;
}
// ghost_record of p packed pairs from n starts, as the kernel calls it; have: n bytes (the main record has weight); out: n x p x 8
extern "C" int zgh_records(int model, int count, const float *rows, int stop, float user, const float *media, int p, const uint32_t *pairs,
                           int n, const float *lambda, const float *o, const float *d, const unsigned char *have, float *out)
{
    GhostTable G; GhostMedia M;
    tables(model, count, rows, stop, user, media, G, M);
    const GhostTable *GP = &G; const GhostMedia *MP = &M;
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < p; ++j)
            put(out + 8 * (static_cast<size_t>(r) * p + j), ghost_record(GP, MP, pairs[j], have[r] != 0, lambda[r], V3{o[3 * r], o[3 * r + 1], o[3 * r + 2]},
                                                                         V3{d[3 * r], d[3 * r + 1], d[3 * r + 2]}));
    return G.model;
}
// the pinned STRICT path from the same starts: surf count x (center, radius2, sign, housing2); out: n x 7 (o, d as the trace leaves
// them, 1.0 where it passes)
extern "C" int zgh_strict(int count, const float *surf, const float *disp, int n, const float *lambda, const float *o, const float *d, float *out)
{
    Surface S[kMaxSurfaces] = {};
    SpectralTable W = {};
    W.count = count;
    for (int i = 0; i < count; ++i) {
        S[i].center = surf[4 * i]; S[i].radius2 = surf[4 * i + 1]; S[i].sign = surf[4 * i + 2]; S[i].housing2 = surf[4 * i + 3];
        W.iorD[i] = disp[2 * i]; W.cauchyB[i] = disp[2 * i + 1];
    }
    const Surface *SP = S; const SpectralTable *WP = &W;
    int passed = 0;
    for (int r = 0; r < n; ++r) {
        V3 po{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, pd{d[3 * r], d[3 * r + 1], d[3 * r + 2]};
        uint32_t tir = 0;
        const bool ok = trace_lens_spectral_strict(SP, WP, count, spectral_dl(lambda[r]), po, pd, tir);
        passed += ok ? 1 : 0;
        float *q = out + 7 * r;
        q[0] = po.x; q[1] = po.y; q[2] = po.z; q[3] = pd.x; q[4] = pd.y; q[5] = pd.z; q[6] = ok ? 1.0f : 0.0f;
    }
    return passed;
}
"""


def ghost():
    """zgh_trace (run_ghost_trace), zgh_records (run_ghost_records), zgh_strict"""
    return _build("ghost", GHOST)


def _tables_args(L, disp, film):
    count = L["count"]
    rows = np.stack([L["radius"], L["thickness"], L["aperture"]], 1)
    fl = (np.zeros(count, F32), np.zeros(count, F32)) if film is None else film
    media = np.stack([disp["ior_d"], disp["cauchy_b"], fl[0], fl[1]], 1)
    return [np.ascontiguousarray(a, F32) for a in (rows, media)]


def run_ghost_trace(drv, L, disp, lam, o, d, a, b, film=None, model=1):
    """(n, 8) float32 records of ghost_trace for one pair ((-1, -1): the plain path); L = ghost_ref.lens(info)"""
    fp = ctypes.POINTER(ctypes.c_float)
    keep = _tables_args(L, disp, film) + [np.ascontiguousarray(v, F32) for v in (lam, o, d)]
    n = len(keep[3])
    out = np.full((n, 8), np.nan, F32)
    drv.zgh_trace(int(model), L["count"], keep[0].ctypes.data_as(fp), int(L["stop"]), ctypes.c_float(float(L["user"])), keep[1].ctypes.data_as(fp),
                  int(a), int(b), n, keep[2].ctypes.data_as(fp), keep[3].ctypes.data_as(fp), keep[4].ctypes.data_as(fp), out.ctypes.data_as(fp))
    return out


def run_ghost_records(drv, L, disp, lam, o, d, pairs, have=None, film=None, model=1):
    """(n, p, 8) float32 records of ghost_record, the call's columns: pairs (p, 2) of (a, b) or (p,) packed, have (n,) bool"""
    fp = ctypes.POINTER(ctypes.c_float)
    keep = _tables_args(L, disp, film) + [np.ascontiguousarray(v, F32) for v in (lam, o, d)]
    n = len(keep[3])
    pairs = np.asarray(pairs)
    packed = np.ascontiguousarray(pairs if pairs.ndim == 1 else pairs[:, 0].astype(np.uint32) | (pairs[:, 1].astype(np.uint32) << 8), np.uint32)
    hv = np.ones(n, np.uint8) if have is None else np.ascontiguousarray(have, np.uint8)
    out = np.full((n, len(packed), 8), np.nan, F32)
    drv.zgh_records(int(model), L["count"], keep[0].ctypes.data_as(fp), int(L["stop"]), ctypes.c_float(float(L["user"])), keep[1].ctypes.data_as(fp),
                    len(packed), packed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, keep[2].ctypes.data_as(fp), keep[3].ctypes.data_as(fp),
                    keep[4].ctypes.data_as(fp), hv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.ctypes.data_as(fp))
    return out


def split_ghost(rec):
    """(origin, dir, weight, flags, reason, interface, leg) of records (..., 8)"""
    flags = bits_f32(rec[..., 7])
    traced = (flags & 1) != 0
    reason = np.where(traced, 0, (flags >> 8) & 0xF).astype(np.int64)
    return rec[..., 0:3], rec[..., 3:6], rec[..., 6], flags, reason, ((flags >> 16) & 0x3F).astype(np.int64), ((flags >> 24) & 3).astype(np.int64)


# ---- csrc/traceback.hpp ---------------------------------------------------------------------------------------------------------
TRACEBACK = r"""
#include "traceback.hpp"
extern "C" int zt_trace(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior, const float *aperture,
                        int apertureElement, float userApertureRadius, float originShift, float sensorWidth, int useLUT, int lutSize, int domain,
                        float apertureRadius, float focalDistance, int useDof, float ovDistance, float ovRadius,
                        long n, const float *o, const float *d, float *screen, unsigned *flags)
{
    zoic::TraceBackTable T;
    zoic::fill_traceback_table(T, model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius, originShift,
                               sensorWidth, useLUT != 0, lutSize, domain != 0, apertureRadius, focalDistance, useDof != 0, ovDistance, ovRadius);
    for (long i = 0; i < n; ++i)
        flags[i] = zoic::trace_back_ray(T, o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2], screen[2 * i], screen[2 * i + 1]);
    return 0;
}
"""


def traceback():
    """zt_trace, called through drive_traceback"""
    return _build("traceback", TRACEBACK)


def drive_traceback(driver, cam, p, o, d):
    info = cam.info()
    n = info["lensCount"]
    el = [np.ascontiguousarray(info["elements"][:, k], dtype=np.float32) for k in range(4)]
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    scr = np.zeros((len(o), 2), np.float32)
    fl = np.zeros(len(o), np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    F = ctypes.c_float
    driver.zt_trace(int(p["lensModel"]), F(info["tan_fov"]), n, P(el[0]), P(el[1]), P(el[2]), P(el[3]), info["apertureElement"],
                    F(info["userApertureRadius"]), F(info["originShift"]), F(p["sensorWidth"]),
                    int(bool(p["kolbSamplingLUT"]) and len(info["lutKeys"]) > 0), len(info["lutKeys"]), int(not info["fastRunsStrict"]),
                    F(info["apertureRadius"]), F(p["focalDistance"]), int(bool(p["useDof"])), F(p.get("opticalVignettingDistance", 0.0)),
                    F(p.get("opticalVignettingRadius", 1.0)), ctypes.c_long(len(o)), P(o), P(d), P(scr), P(fl))
    return scr, fl


# ---- csrc/reverse.hpp -----------------------------------------------------------------------------------------------------------
REVERSE = r"""
#include "reverse.hpp"
extern "C" int zr_project(int model, float tanFov, int count, const float *radius, const float *thickness, const float *ior, const float *aperture,
                          int apertureElement, float userApertureRadius, float originShift, float sensorWidth, int useLUT, int lutSize, int domain,
                          long n, const float *pts, float *screen, unsigned *flags)
{
    zoic::ReverseTable T;
    zoic::fill_reverse_table(T, model, tanFov, count, radius, thickness, ior, aperture, apertureElement, userApertureRadius, originShift,
                             sensorWidth, useLUT != 0, lutSize, domain != 0);
    for (long i = 0; i < n; ++i) flags[i] = zoic::project_point(T, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], screen[2 * i], screen[2 * i + 1]);
    return 0;
}
"""


def reverse():
    """zr_project, called through drive_reverse"""
    return _build("reverse", REVERSE)


def drive_reverse(driver, cam, p, pts):
    """the host build on points (m,3): (screen (m,2), flags (m,))"""
    info = cam.info()
    n = info["lensCount"]
    el = [np.ascontiguousarray(info["elements"][:, k], dtype=np.float32) for k in range(4)]
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    scr = np.zeros((len(pts), 2), np.float32)
    fl = np.zeros(len(pts), np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    model = p["lensModel"]
    domain = not info["fastRunsStrict"]
    driver.zr_project(model, ctypes.c_float(info["tan_fov"]), n, P(el[0]), P(el[1]), P(el[2]), P(el[3]), info["apertureElement"],
                      ctypes.c_float(info["userApertureRadius"]), ctypes.c_float(info["originShift"]), ctypes.c_float(p["sensorWidth"]),
                      int(bool(p["kolbSamplingLUT"]) and len(info["lutKeys"]) > 0), len(info["lutKeys"]), int(domain), ctypes.c_long(len(pts)), P(pts), P(scr), P(fl))
    return scr, fl

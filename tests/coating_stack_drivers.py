"""Host builds of csrc/coating_stack.hpp and of the stack-aware paths of csrc/ghost.hpp for the tests, through host_drivers._build: the
interface function, the two phase polynomials, the forward path and the ghost tracer under the coating policy `const StackTable *`.
The trace-back and splat side needs no driver: its host calls are in the C-ABI.  A helper, not a test."""
import ctypes

import numpy as np

import host_drivers
from coating_stack_ref import MAX_LAYERS, table

F32 = np.float32
FP = ctypes.POINTER(ctypes.c_float)
IP = ctypes.POINTER(ctypes.c_int32)

SOURCE = r"""
#include "coating_stack.hpp"
#include "ghost.hpp"
using namespace zoic;
// layers: count; index, thickness: count x 8; trace order, layers as a forward ray meets them
static void stacks(int count, const int32_t *layers, const float *index, const float *thickness, StackTable &K)
{
    K = StackTable{};
    for (int i = 0; i < count && i < kMaxSurfaces; ++i) {
        K.layers[i] = layers[i];
        for (int l = 0; l < kCoatingMaxLayers; ++l) K.layer[i][l] = StackLayer{index[8 * i + l], thickness[8 * i + l]};
    }
}
extern "C" void zcs_sincos(int n, const float *x, float *s, float *c, float *s2, float *c2)
{
    for (int i = 0; i < n; ++i) { s[i] = film_sinpi(x[i]); c[i] = film_cospi(x[i]); film_sincospi(x[i], s2[i], c2[i]); }
}
// n interfaces n1 -> n2 at (ci, ct, lambda) through ONE stack of L layers given in the table's order; forward: met in that order
extern "C" void zcs_interface(int n, const float *n1, const float *n2, const float *ci, const float *ct, const float *lambda, int L,
                              const float *index, const float *thickness, int forward, float nc, float lambda0, float *T)
{
    StackTable K = {};
    K.layers[0] = L;
    for (int l = 0; l < L; ++l) K.layer[0][l] = StackLayer{index[l], thickness[l]};
    const StackTable *KP = &K;
    for (int r = 0; r < n; ++r) T[r] = coated_transmittance(KP, 0, forward != 0, n1[r], n2[r], ci[r], ct[r], nc, lambda0, lambda[r]);
}
// ztr_trace of host_drivers.TRANSMITTANCE under the stacks
extern "C" int zcs_trace(int count, const float *surf, const float *disp, const float *film, const int32_t *layers, const float *index,
                         const float *thickness, int n, const float *lambda, const float *o, const float *d, float *T)
{
    Surface S[kMaxSurfaces] = {};
    SpectralTable W = {};
    FilmTable F = {};
    StackTable K;
    stacks(count, layers, index, thickness, K);
    W.count = F.count = count;
    for (int i = 0; i < count; ++i) {
        S[i].center = surf[4 * i]; S[i].radius2 = surf[4 * i + 1]; S[i].sign = surf[4 * i + 2]; S[i].housing2 = surf[4 * i + 3];
        W.iorD[i] = disp[2 * i]; W.cauchyB[i] = disp[2 * i + 1];
        F.index[i] = film[2 * i]; F.lambda0[i] = film[2 * i + 1];
    }
    const Surface *SP = S;
    const SpectralTable *WP = &W;
    const FilmTable *FP = &F;
    const StackTable *KP = &K;
    for (int r = 0; r < n; ++r)
        T[r] = path_transmittance(SP, WP, FP, KP, count, lambda[r], V3{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, V3{d[3 * r], d[3 * r + 1], d[3 * r + 2]});
    return 0;
}
// zgh_records of host_drivers.GHOST under the stacks; a < 0: ghost_trace of the plain path, p == 1
extern "C" int zcs_ghosts(int count, const float *rows, int stop, float user, const float *media, const int32_t *layers, const float *index,
                          const float *thickness, int p, const uint32_t *pairs, int plain, int n, const float *lambda, const float *o,
                          const float *d, const unsigned char *have, float *out)
{
    float radius[kMaxSurfaces] = {}, thick[kMaxSurfaces] = {}, aperture[kMaxSurfaces] = {};
    GhostTable G; GhostMedia M = GhostMedia{};
    StackTable K;
    stacks(count, layers, index, thickness, K);
    for (int i = 0; i < count && i < kMaxSurfaces; ++i) {
        radius[i] = rows[3 * i]; thick[i] = rows[3 * i + 1]; aperture[i] = rows[3 * i + 2];
        M.iorD[i] = media[4 * i]; M.cauchyB[i] = media[4 * i + 1]; M.filmIndex[i] = media[4 * i + 2]; M.filmLambda0[i] = media[4 * i + 3];
    }
    fill_ghost_table(G, 1, count, radius, thick, aperture, stop, user);
    const GhostTable *GP = &G; const GhostMedia *MP = &M; const StackTable *KP = &K;
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < p; ++j) {
            const V3 o0{o[3 * r], o[3 * r + 1], o[3 * r + 2]}, d0{d[3 * r], d[3 * r + 1], d[3 * r + 2]};
            const GhostRay g = plain ? ghost_trace(GP, MP, -1, -1, lambda[r], o0, d0, KP) : ghost_record(GP, MP, pairs[j], have[r] != 0, lambda[r], o0, d0, KP);
            float *q = out + 8 * (static_cast<size_t>(r) * p + j);
            q[0] = g.ox; q[1] = g.oy; q[2] = g.oz; q[3] = g.dx; q[4] = g.dy; q[5] = g.dz; q[6] = g.weight;
            __builtin_memcpy(q + 7, &g.flags, 4);
        }
    return G.model;
}
"""


def driver():
    """zcs_sincos, zcs_interface (run_interface), zcs_trace (run_transmittance), zcs_ghosts (run_ghost_records)"""
    return host_drivers._build("coating_stack", SOURCE)


def _f(a):
    return np.ascontiguousarray(a, F32)


def sincos(drv, x):
    """(film_sinpi, film_cospi, film_sincospi's sine, its cosine) of x, float32"""
    x = _f(x)
    out = [np.zeros_like(x) for _ in range(4)]
    drv.zcs_sincos(len(x), x.ctypes.data_as(FP), *[a.ctypes.data_as(FP) for a in out])
    return out


def run_interface(drv, n1, n2, ci, ct, lam, layers, forward=True, film=(0.0, 0.0)):
    """(n,) float32 T_i of coated_transmittance through `layers` ((index, nm) in the TABLE's order: as a forward ray meets them;
    forward False: the ray meets them backwards; empty: the film entry `film`, or bare)"""
    args = [_f(a).reshape(-1) for a in np.broadcast_arrays(n1, n2, ci, ct, lam)]
    idx, thk = _f([p[0] for p in layers] + [0.0]), _f([p[1] for p in layers] + [0.0])
    T = np.full(len(args[0]), -1.0, F32)
    drv.zcs_interface(len(T), *[a.ctypes.data_as(FP) for a in args], len(layers), idx.ctypes.data_as(FP), thk.ctypes.data_as(FP),
                      int(bool(forward)), ctypes.c_float(film[0]), ctypes.c_float(film[1]), T.ctypes.data_as(FP))
    return T


def _table_args(stacks_trace_order):
    layers, index, thick = table(stacks_trace_order)
    keep = [np.ascontiguousarray(layers, np.int32), _f(index), _f(thick)]
    return keep, [keep[0].ctypes.data_as(IP), keep[1].ctypes.data_as(FP), keep[2].ctypes.data_as(FP)]


def run_transmittance(drv, surf, disp, lam, o, d, stacks_trace_order, film=None, housing2=None):
    """host_drivers.run_transmittance under stacks (trace order, layers as a forward ray meets them; None entries: no stack)"""
    n, count = len(o), len(surf)
    h2 = np.full(count, np.inf, F32) if housing2 is None else np.asarray(housing2, F32)
    s4 = np.stack([surf[:, 0], surf[:, 1], surf[:, 2], h2], 1)
    fl = np.zeros((count, 2), F32) if film is None else np.stack([film[0], film[1]], 1)
    keep = [_f(a) for a in (s4, np.stack([disp["ior_d"], disp["cauchy_b"]], 1), fl, lam, o, d)]
    c = [a.ctypes.data_as(FP) for a in keep]
    tk, tc = _table_args(stacks_trace_order)
    T = np.full(n, -1.0, F32)
    assert drv.zcs_trace(count, c[0], c[1], c[2], *tc, n, c[3], c[4], c[5], T.ctypes.data_as(FP)) == 0
    return T


def run_ghost_records(drv, L, disp, lam, o, d, pairs, stacks_trace_order, have=None, film=None):
    """host_drivers.run_ghost_records under stacks; pairs None: the plain path, (n, 1, 8)"""
    keep = host_drivers._tables_args(L, disp, film) + [_f(v) for v in (lam, o, d)]
    n = len(keep[3])
    plain = pairs is None
    pairs = np.zeros((1, 2), np.int64) if plain else np.asarray(pairs)
    packed = np.ascontiguousarray(pairs if pairs.ndim == 1 else pairs[:, 0].astype(np.uint32) | (pairs[:, 1].astype(np.uint32) << 8), np.uint32)
    hv = np.ones(n, np.uint8) if have is None else np.ascontiguousarray(have, np.uint8)
    tk, tc = _table_args(stacks_trace_order)
    out = np.full((n, len(packed), 8), np.nan, F32)
    drv.zcs_ghosts(L["count"], keep[0].ctypes.data_as(FP), int(L["stop"]), ctypes.c_float(float(L["user"])), keep[1].ctypes.data_as(FP), *tc,
                   len(packed), packed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), int(plain), n, keep[2].ctypes.data_as(FP),
                   keep[3].ctypes.data_as(FP), keep[4].ctypes.data_as(FP), hv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.ctypes.data_as(FP))
    return out

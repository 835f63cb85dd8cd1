"""What the tests of the trace-back transmittance share (zoic_amd/csrc/traceback_throughput.hpp): the f64 restatement, the ray sets,
and the per-item host calls.  A helper, not a test.

Restatement.  traceback_ref.TraceBack's trace in absolute coordinates (the reference's spheres about their centres), with
backward_spectral_ref's media -- the f32 indices of the definition promoted to f64 -- and, at every interface front to rear,
transmittance_ref.interface_transmittance (f64) on that interface's |cos i|, cos t = sqrt|1 - eta^2 (1 - cos^2 i)| and its two indices,
under the film of that interface (trace order).  Which rays are traced is TraceBack.trace's business: this loop ends nothing and its T
means something only where that trace says `traced`.

Forward.  transmittance_ref.transmittance on the start of a record's accepted try (differentials_ref.kolb_start): the forward f64 T
that reciprocity compares with."""
import ctypes

import numpy as np

from zoic_amd import ZoicCamera, _capi

import backward_spectral_ref as bs
import differentials_ref as dref
import machine_lens_corpus as mc
import traceback_cases as tc
import transmittance_ref as tref
from traceback_ref import RAYTRACED

F32 = np.float32
LAMBDA_D32 = F32(587.5618)
MAX_RECORDS = 8192      # the live forward records of a traceback_cases frame the per-ray host calls are given (a stride)
# tests/test_traceback_throughput_cpu.py measures these and says how (its docstring has the tables): the largest |T_host - T_f64| of
# its runs, the bound asserted wherever "the bound" is said (4 x it: the margin for other compilers' host builds), and the largest
# E_rec = |T_back_f64(record) - T_fwd_f64(start)|, reference against reference
MEASURED = 5.695e-7
BOUND = 4 * MEASURED
E_REC = 7.33e-8


class Throughput(bs.SpectralTraceBack):
    """SpectralTraceBack with the transmittance of the path: films = (index, lambda0) in trace order, or None: bare"""

    def __init__(self, info, params, dispersion, films=None):
        super().__init__(info, params, dispersion)
        n = max(self.n, 1)
        self.film_index = np.zeros(n) if films is None else np.asarray(films[0], np.float64)
        self.film_lambda0 = np.zeros(n) if films is None else np.asarray(films[1], np.float64)

    def _path(self, o, d, lam, rear, front):
        """T (m,) of the f64 path at ONE wavelength with the media (rear, front); no ray is ended"""
        m = len(o)
        if self.model != RAYTRACED:
            return np.ones(m)
        with np.errstate(all="ignore"):
            q = -o
            b = d / np.sqrt((d * d).sum(1))[:, None]
            T = np.ones(m)
            for i in range(self.n - 1, -1, -1):
                R, C = self.R[i], np.array([0.0, 0.0, self.centre[i]])
                L = C - q
                tca = (L * b).sum(1)
                d2 = (L * L).sum(1) - tca * tca
                thc = np.sqrt(np.abs(R * R - d2))
                hit = q + (tca - thc * np.sign(R))[:, None] * b
                nrm = (hit - C) / R
                cosi = -(b * nrm).sum(1)
                n1, n2 = front[i], rear[i]
                eta = n1 / n2
                ct = np.sqrt(np.abs(1.0 - eta * eta * (1.0 - cosi * cosi)))
                T = T * tref.interface_transmittance(n1, n2, np.abs(cosi), ct, self.film_index[i], self.film_lambda0[i], lam)
                b = eta * b + (eta * cosi - ct)[:, None] * nrm
                q = hit
        return T

    def transmittance(self, origin, direction, lam=None):
        """T (m,) f64 of the rays at wavelength(s) lam (None: the d-line, kLambdaD32); NaN where the wavelength is rejected"""
        o = np.array(origin, np.float64).reshape(-1, 3)
        d = np.array(direction, np.float64).reshape(-1, 3)
        lam = np.broadcast_to(np.asarray(LAMBDA_D32 if lam is None else lam, F32), (len(o),))
        out = np.full(len(o), np.nan)
        ok = bs.valid(lam)
        for l in np.unique(lam[ok]):
            pick = ok & (lam == l)
            rear, front = bs.media(self.dispersion, l) if self.model == RAYTRACED else (None, None)
            out[pick] = self._path(o[pick], d[pick], float(l), rear, front)
        return out


def forward_transmittance(info, disp, o0, d0, lam, films=None):
    """the forward f64 T of the starts (o0, d0) at wavelength lam (a scalar): transmittance_ref.transmittance; (T, passes)"""
    surf = dref.surfaces(info)
    return tref.transmittance(surf, disp, np.full(len(o0), float(lam)), o0, d0, *(films or (None, None)))


# ---- the per-item host calls --------------------------------------------------------------------------------------------------------
def lib_throughput(cam, o, d, lam=None):
    """zoic_trace_back_ray_transmittance (lam None) or its _spectral form on every ray: (ps (m,2) f32, flags (m,) u32, T (m,) f32)"""
    lib, h = _capi.load(), cam._h
    m = len(o)
    ps, fl, T = np.zeros((m, 2), F32), np.zeros(m, np.uint32), np.full(m, -1.0, F32)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    V, FP, UP = ctypes.POINTER(_capi.Vec3), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    po, pd, pp, pf, pt = o.ctypes.data, d.ctypes.data, ps.ctypes.data, fl.ctypes.data, T.ctypes.data
    lam = None if lam is None else np.broadcast_to(np.asarray(lam, F32), (m,))
    dline, spectral = lib.zoic_trace_back_ray_transmittance, lib.zoic_trace_back_ray_transmittance_spectral
    for i in range(m):
        a = (ctypes.cast(po + 12 * i, V), ctypes.cast(pd + 12 * i, V))
        t = (ctypes.cast(pp + 8 * i, FP), ctypes.cast(pf + 4 * i, UP), ctypes.cast(pt + 4 * i, FP))
        rc = dline(h, *a, *t) if lam is None else spectral(h, *a, float(lam[i]), *t)
        assert rc == 0, rc
    return ps, fl, T


def coat(cam, films):
    """the camera with films (index, lambda0 in TRACE order, or None: bare) on it"""
    if films is None:
        cam.set_coatings(None, None)
    else:
        cam.set_coatings(np.asarray(films[0], F32)[::-1], np.asarray(films[1], F32)[::-1])   # file order
    return cam


# ---- the ray sets of the accuracy and reciprocity tests ------------------------------------------------------------------------------
class Lens:
    """One lens of the accuracy tests: its tables-only camera, a stride of the oracle's live d-line records (at most MAX_RECORDS; the
    corpus lenses: the leading live records of machine_lens_corpus.ray_set) and the starts of their accepted tries.  name: a
    traceback_cases configuration (C2 ... C5, given bs.DISPERSIVE's V-numbers) or a corpus lens."""

    def __init__(self, oracle_lib, name):
        self.name = name
        corpus = name in mc.BY_NAME
        s, st = tc.frame_samples()
        if corpus:
            self.cam, self.p = mc.camera(name)
            rays, lead = mc.ray_set(oracle_lib, self.cam, name)
            _, o, d, w = mc.oracle_records(oracle_lib, name)
            rows = mc.strided(np.flatnonzero(w > 0), 3072)
            assert len(rows) == lead and np.array_equal(rays[:lead, 0:3], o[rows].astype(F32))
            tries = mc.oracle_tries(oracle_lib, name)[rows]
            oc = mc.oracle_camera(oracle_lib, name)
        else:
            self.p = tc.params_of(name)
            self.cam = bs.set_dispersion(tc.update(ZoicCamera(device=-1), self.p), name)
            oc = tc.update(oracle_lib.OracleCamera(), self.p)
            r = oc.create_rays(s, rng_states=st)
            o, d, w = r["origin"].T, r["dir"].T, r["weight"]
            rows = mc.strided(np.flatnonzero(w > 0), MAX_RECORDS)
            tries = r["tries"].astype(np.int64)[rows]
        self.o, self.d = np.ascontiguousarray(o[rows], F32), np.ascontiguousarray(d[rows], F32)
        self.o0, self.d0 = dref.kolb_start(oc, self.p, s[rows], tries, st[rows], oracle_lib)
        oc.close()
        self.info, self.disp = self.cam.info(), self.cam.dispersion()
        self.films = tref.films_where_media_differ(self.disp)
        self._ref = {}

    def reference(self, lam, coated):
        """(f64 trace-back dict, edge set, f64 T) of the records at wavelength lam (None: the d-line), cached"""
        key = (lam, coated)
        if key not in self._ref:
            R = Throughput(self.info, self.p, self.disp, self.films if coated else None)
            ref = R.trace(self.o, self.d) if lam is None else R.trace_at(self.o, self.d, lam)
            self._ref[key] = ref, R.edge(ref), R.transmittance(self.o, self.d, lam)
        return self._ref[key]


_LENSES = {}


def lens(oracle_lib, name):
    if name not in _LENSES:
        _LENSES[name] = Lens(oracle_lib, name)
    return _LENSES[name]


CONFIGS = ("C2", "C3", "C4", "C5")
LENSES = CONFIGS + tuple(mc.ACCURACY)
WAVELENGTHS = (None,) + bs.LAMBDAS      # None: the d-line calls; then 400, 486.1327, 656.2725 and 700 nm

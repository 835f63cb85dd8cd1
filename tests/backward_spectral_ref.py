"""numpy f64 restatement of the two backward paths at a wavelength per item (zoic_amd/csrc/backward_spectral.hpp), written from the
definition: the trace of traceback_ref.py (absolute coordinates, the reference's spheres about their centres) and the chief ray through
the stop's centre on reverse_ref.py's meridional interfaces, with the media's indices at each item's wavelength.  The indices are the f32 numbers the definition
names -- spectral_ref.spectral_iors on the camera's dispersion(), promoted to f64 -- so what is measured against this file is the
trace, not the rounding of an index; the ratio of two media is taken in f64.

Items are grouped by wavelength and each group runs through the d-line restatement's own code with that group's indices."""
import numpy as np

from reverse_ref import Lens
from spectral_ref import spectral_iors
from traceback_ref import RAYTRACED, TraceBack

F32 = np.float32
TB_WAVELENGTH, PROJECT_WAVELENGTH = 8, 6
LAMBDA_MIN, LAMBDA_MAX = F32(360.0), F32(830.0)


def valid(lam):
    lam = np.asarray(lam, F32)
    with np.errstate(invalid="ignore"):
        return (lam >= LAMBDA_MIN) & (lam <= LAMBDA_MAX)   # False for NaN


def media(dispersion, lam):
    """(index behind interface i, index in front of it) at wavelength lam, trace order, f64 copies of the f32 indices"""
    n = spectral_iors(dispersion["ior_d"], dispersion["cauchy_b"], lam)
    return n.astype(np.float64), np.append(n[1:], F32(1)).astype(np.float64)


class SpectralTraceBack(TraceBack):
    """TraceBack at a wavelength per ray: dispersion = ZoicCamera.dispersion()"""

    def __init__(self, info, params, dispersion):
        super().__init__(info, params)
        self.dispersion = dispersion

    def trace_at(self, origin, direction, lam):
        """lam: a scalar or (m,) float32, nm.  The dict of TraceBack.trace; a ray whose wavelength is rejected has traced False, reason
        TB_WAVELENGTH, ps 0 and no clearances."""
        o = np.array(origin, np.float64).reshape(-1, 3)
        d = np.array(direction, np.float64).reshape(-1, 3)
        lam = np.broadcast_to(np.asarray(lam, F32), (len(o),))
        out = self.trace(o, d)   # (shapes; every row is overwritten below)
        ok = valid(lam)
        for key in ("ps", "clear", "other"):
            out[key][~ok] = 0.0 if key == "ps" else np.nan
        out["traced"][~ok] = False
        out["reason"][~ok] = TB_WAVELENGTH
        out["iface"][~ok] = -1
        out["clearance"][~ok] = np.inf
        out["cap"][~ok] = np.inf
        out["past_lut"][~ok] = False
        d_line = self.ior_rear, self.ior_front
        try:
            for l in np.unique(lam[ok]):
                pick = ok & (lam == l)
                if self.model == RAYTRACED:
                    self.ior_rear, self.ior_front = media(self.dispersion, l)
                res = self.trace(o[pick], d[pick])
                for key in out:
                    out[key][pick] = res[key]
        finally:
            if self.model == RAYTRACED:
                self.ior_rear, self.ior_front = d_line
        return out


class SpectralLens(Lens):
    """reverse_ref.Lens with the indices of one wavelength"""

    def __init__(self, info, sensor_width, dispersion, lam):
        super().__init__(info, sensor_width)
        self.ior_rear, self.ior_front = media(dispersion, lam)


def chief_through(L, rq, zq, grid=400, halvings=70):
    """The definition's chief ray, in f64: for points (rq > 0, zq) of the meridional plane (trace frame) the sine s of the angle at which
    the ray through the point leaves the centre of the stop of Lens L towards the front.  G(s) = the signed distance of the point from
    the line of the ray after the front group; the root taken is the one continuous with the axis: the first change of sign of G met
    from s = 0 outwards (on a grid of `grid` sines per side, between two rays that both get out), closed in by bisection.  Returns
    (sensor height along rq, found (m,) bool)."""
    rq = np.asarray(rq, np.float64)
    zq = np.asarray(zq, np.float64)
    front = list(range(L.stop + 1, L.n))
    zs = L.vtx[L.stop]

    def G(s):
        x, z, ur, uz, ok, _ = L.trace(front, np.zeros_like(s), np.full_like(s, zs), s, np.sqrt(1.0 - s * s), True)
        a, b = rq - x, zq - z
        ok = ok & (ur * a + uz * b > 0.0)
        return np.where(ok, ur * b - uz * a, np.nan)

    m = len(rq)
    lo, hi, found = np.zeros(m), np.zeros(m), np.zeros(m, bool)
    with np.errstate(invalid="ignore"):
        for sign in (1.0, -1.0):
            prev_s, prev_g = np.zeros(m), G(np.zeros(m))
            for k in range(1, grid):
                sk = np.full(m, sign * 0.999 * k / grid)
                gk = G(sk)
                hit = ~found & np.isfinite(prev_g) & np.isfinite(gk) & (np.sign(prev_g) != np.sign(gk)) & (prev_g != 0.0)
                lo[hit], hi[hit] = prev_s[hit], sk[hit]
                found |= hit
                prev_s, prev_g = sk, gk
        glo = G(lo)
        for _ in range(halvings):
            mid = 0.5 * (lo + hi)
            gm = G(mid)
            left = np.sign(gm) == np.sign(glo)
            lo, glo = np.where(left, mid, lo), np.where(left, gm, glo)
            hi = np.where(left, hi, mid)
    s = 0.5 * (lo + hi)
    x, z, ur, uz, ok, _ = L.trace(range(L.stop, -1, -1), np.zeros(m), np.full(m, zs), -s, -np.sqrt(1.0 - s * s), False)
    t = (L.origin_shift - z) / uz
    return x + t * ur, found & ok


def project_at(info, sensor_width, dispersion, points, lam):
    """The f64 projection of points (m,3) (the frame of the records, in front of the lens) at one wavelength: (ps (m,2), ok (m,)): the
    sensor point of the chief ray through each point (chief_through), over sensorWidth / 2; a point on the axis gives (0, 0)."""
    L = SpectralLens(info, sensor_width, dispersion, lam)
    q = -np.asarray(points, np.float64).reshape(-1, 3)
    rq = np.hypot(q[:, 0], q[:, 1])
    off = rq > 0
    xs, ok = np.zeros(len(q)), np.ones(len(q), bool)
    xs[off], ok[off] = chief_through(L, rq[off], q[off, 2])
    ca = np.where(off, q[:, 0] / np.where(off, rq, 1.0), 0.0)
    sa = np.where(off, q[:, 1] / np.where(off, rq, 1.0), 0.0)
    return np.stack([xs * ca, xs * sa], 1) / L.half_sensor, ok


# ---- inputs shared by tests/test_backward_spectral_cpu.py and tests/test_backward_spectral_gpu.py ------------------------------
LAMBDA_D = 587.5618
LAMBDAS = (400.0, 486.1327, 656.2725, 700.0)                       # the accuracy wavelengths (nm)
REJECTED = (359.99, 830.01, np.nan, np.inf, -np.inf, -1.0, 0.0)    # wavelengths every call refuses
# configuration (traceback_cases.CONFIGS) -> the V-number given to every glass, None: the prescription's own fifth column
DISPERSIVE = {"C2": None, "C5": None, "C3": 50.0, "C4": 50.0, "triplet": 50.0}


def set_dispersion(cam, name):
    """the dispersion the tests give configuration `name` (after the camera's update)"""
    v = DISPERSIVE.get(name)
    if v is not None:
        cam.set_abbe_numbers(np.full(cam.info()["lensCount"], v, F32))
    return cam


def trace_back_rays(tc, info, records, raytraced, per_family=512):
    """The trace-back ray sets of one configuration, concatenated: (origin (m,3) f32, dir (m,3) f32).  records = (origin, dir, weight)
    of the oracle's frame; for a RAYTRACED camera the rejection families made from live records, random and dyadic lines are added,
    for every camera the non-finite rays and random lines."""
    o, d, w = records
    O, D = [o.astype(F32)], [d.astype(F32)]
    if raytraced:
        live = np.flatnonzero(w > 0)[:: max(1, int((w > 0).sum()) // per_family)]
        for fo, fd in tc.rejection_families(info, o[live], d[live]).values():
            O.append(fo); D.append(fd)
        dy_o, dy_d = tc.dyadic_lines(info, per_family)
        for t in (0.0, 10.0, 10000.0):
            O.append((dy_o - t * dy_d).astype(F32)); D.append(dy_d.astype(F32))
    nf_o, nf_d = tc.non_finite_rays()
    rl_o, rl_d = tc.random_lines(info, 4 * per_family)
    O += [nf_o, rl_o]; D += [nf_d, rl_d]
    return np.ascontiguousarray(np.concatenate(O), F32), np.ascontiguousarray(np.concatenate(D), F32)


def mixed_wavelengths(m, seed=17):
    """(m,) float32: valid wavelengths (uniform in [360, 830], the ends and the d-line among them) with every fourth item one of the
    rejected values -- valid and invalid interleaved inside every wave"""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(360.0, 830.0, m).astype(F32)
    lam[1::16] = F32(LAMBDA_D)
    lam[5::64] = F32(360.0)
    lam[9::64] = F32(830.0)
    bad = np.array(REJECTED, F32)
    lam[3::4] = bad[np.arange(len(lam[3::4])) % len(bad)]
    return lam

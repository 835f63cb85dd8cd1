"""numpy f64 restatement of the trace-back (include/zoic_amd.h, "trace-back") for the tests, written from the definition and from
ZoicCamera.info() in ABSOLUTE coordinates of the trace frame, the reference's way: every interface a sphere about its centre
(vertex - R, the vertices at computeLensCenters' f32 sums), intersected with raySphereIntersection's tca / thc and its `reverse` root
tca - thc sign(R) (zoic.cpp:973-995), refracted by Snell's law with the true ratio of the two media.  The stop is the reference's
sphere.  Besides the result it reports how far from every clip limit each ray passed, which is what the tests use to leave the rays
out whose accept / reject decision belongs to rounding."""
import numpy as np

F32 = np.float32
AWAY, MISS, CLIPPED, TIR, NON_FINITE, MODEL, OUTSIDE_DOMAIN = 1, 2, 3, 4, 5, 6, 7
THINLENS, RAYTRACED = 0, 1
CAP_SLACK = 2.0 ** -14   # of the front housing radius: how far behind the front element's cap a start point may lie


class TraceBack:
    """info = ZoicCamera.info(), params = the keyword arguments of its update()"""

    def __init__(self, info, params):
        self.model = int(params["lensModel"])
        self.use_dof = bool(params.get("useDof", True))
        self.outside = self.model == RAYTRACED and bool(info["fastRunsStrict"])
        if self.model == THINLENS:
            self.tan_fov = float(info["tan_fov"])
            self.aperture_radius = float(info["apertureRadius"])
            self.focal_distance = abs(float(F32(params["focalDistance"])))
            self.ov_distance = float(F32(params.get("opticalVignettingDistance", 0.0)))
            self.ov_limit = float(F32(info["apertureRadius"]) * F32(params.get("opticalVignettingRadius", 1.0)))
            self.n = 1
            return
        if self.model != RAYTRACED:
            self.n = 0
            return
        el = info["elements"]
        n = self.n = int(info["lensCount"])
        self.stop = int(info["apertureElement"])
        self.R = el[:n, 0].astype(np.float64)
        th = el[:n, 1].astype(F32)
        ior = el[:n, 2].astype(F32)
        vtx = np.zeros(n, F32)
        s = F32(0)
        for i in range(n):
            s = th[0] if i == 0 else F32(s + th[i])
            vtx[i] = s
        self.vtx = vtx.astype(np.float64)
        self.centre = self.vtx - self.R
        self.ior_rear = ior.astype(np.float64)                          # the medium behind interface i
        self.ior_front = np.append(ior[1:], F32(1)).astype(np.float64)  # the medium in front of it
        half = el[:n, 3].astype(np.float64) * 0.5
        h2 = half * half
        ua = F32(info["userApertureRadius"])
        h2[self.stop] = min(h2[self.stop], float(F32(ua * ua)))
        self.housing2 = h2
        self.origin_shift = float(info["originShift"])
        self.half_sensor = float(F32(params["sensorWidth"]) * F32(0.5))
        keys = info["lutKeys"]
        self.last_lut_key = float(keys[-1]) if bool(params.get("kolbSamplingLUT", True)) and len(keys) else None

    def trace(self, origin, direction):
        """origin, direction: (m,3), the frame of the records.  Returns a dict: ps (m,2) (0 where not traced), traced (m,) bool,
        reason (m,), iface (m,) (-1 where none), clear (m, interfaces) = 1 - h^2 / housing2 at every interface the ray reached (NaN
        elsewhere; the thin lens has one column, the least of its aperture and vignetting clearances), clearance (m,) = the least of
        them (+inf if none), cap (m,) = (start z - the front cap's z) / the front housing radius (RAYTRACED; +inf elsewhere), other
        (m, interfaces) = the nearer to 0 of the sphere-miss margin 1 - d2 / R^2 and the Snell term 1 - eta^2 (1 - cos^2) there."""
        o = np.array(origin, np.float64).reshape(-1, 3)
        d = np.array(direction, np.float64).reshape(-1, 3)
        m = len(o)
        ps = np.zeros((m, 2))
        reason = np.zeros(m, int)
        iface = np.full(m, -1)
        clear = np.full((m, max(self.n, 1)), np.nan)
        other = np.full((m, max(self.n, 1)), np.nan)
        cap = np.full(m, np.inf)
        live = np.ones(m, bool)

        def end(mask, why, at=-1):
            mask = mask & live
            reason[mask] = why
            iface[mask] = at
            live[mask] = False

        every = np.ones(m, bool)
        if self.model not in (THINLENS, RAYTRACED) or (self.model == THINLENS and not self.use_dof):
            end(every, MODEL)
        if self.outside:
            end(every, OUTSIDE_DOMAIN)
        with np.errstate(all="ignore"):
            norm = np.sqrt((d * d).sum(1))
            end(~(np.isfinite(o).all(1) & np.isfinite(d).all(1)) | ~(norm > 0), NON_FINITE)
            end(~(d[:, 2] < 0), AWAY)
            o = np.where(live[:, None], o, 0.0)
            b = np.where(live[:, None], d / np.where(norm > 0, norm, 1.0)[:, None], [0.0, 0.0, -1.0])
            if live.any() and self.model == THINLENS:
                end(o[:, 2] > 0, AWAY)
                P = o + (-o[:, 2] / b[:, 2])[:, None] * b
                c1 = 1.0 - (P[:, 0] ** 2 + P[:, 1] ** 2) / self.aperture_radius ** 2
                c = c1
                if self.ov_distance > 0:   # zoic.cpp:1297-1305: |dir * distance - origin| (x, y) < apertureRadius * radius
                    v = b[:, :2] * self.ov_distance - P[:, :2]
                    c = np.minimum(c1, 1.0 - (v * v).sum(1) / self.ov_limit ** 2)
                clear[live, 0] = c[live]
                end((c1 < 0) | ((c <= 0) & (c < c1)), CLIPPED, 0)
                F = P + (-self.focal_distance / b[:, 2])[:, None] * b
                out = F[:, :2] / (self.focal_distance * self.tan_fov)
                end(~np.isfinite(out).all(1), NON_FINITE)
                ps[live] = out[live]
            elif live.any():
                q = -o
                front = self.n - 1
                cf = 1.0 / self.R[front]
                rf = np.sqrt(self.housing2[front])
                h2 = np.minimum(q[:, 0] ** 2 + q[:, 1] ** 2, self.housing2[front])
                capz = -cf * h2 / (1.0 + np.sqrt(np.maximum(1.0 - cf * cf * h2, 0.0)))
                cap = np.where(live, ((q[:, 2] - self.vtx[front]) - capz) / rf, np.inf)
                end(cap < -CAP_SLACK, AWAY)
                for i in range(front, -1, -1):
                    R, C = self.R[i], np.array([0.0, 0.0, self.centre[i]])
                    L = C - q
                    tca = (L * b).sum(1)
                    d2 = (L * L).sum(1) - tca * tca
                    other[live, i] = (1.0 - d2 / (R * R))[live]
                    end(d2 > R * R, MISS, i)
                    thc = np.sqrt(np.abs(R * R - d2))
                    hit = q + (tca - thc * np.sign(R))[:, None] * b
                    hh = hit[:, 0] ** 2 + hit[:, 1] ** 2
                    clear[live, i] = (1.0 - hh / self.housing2[i])[live]
                    end(hh > self.housing2[i], CLIPPED, i)
                    nrm = (hit - C) / R
                    cosi = -(b * nrm).sum(1)
                    eta = self.ior_front[i] / self.ior_rear[i]
                    k2 = 1.0 - eta * eta * (1.0 - cosi * cosi)
                    other[live, i] = np.where(np.abs(k2) < np.abs(other[:, i]), k2, other[:, i])[live]
                    end(k2 < 0, TIR, i)
                    b = eta * b + (eta * cosi - np.sqrt(np.abs(k2)))[:, None] * nrm
                    q = hit
                    q = np.where(live[:, None], q, 0.0)
                    b = np.where(live[:, None], b, [0.0, 0.0, -1.0])
                end(~(b[:, 2] < 0), MISS, 0)
                t = (self.origin_shift - q[:, 2]) / b[:, 2]
                out = (q + t[:, None] * b)[:, :2] / self.half_sensor
                end(~np.isfinite(out).all(1), NON_FINITE)
                ps[live] = out[live]
        with np.errstate(all="ignore"):
            clearance = np.where(np.isnan(clear).all(1), np.inf, np.nanmin(np.where(np.isnan(clear), np.inf, clear), axis=1))
        past = np.zeros(m, bool)   # flag bit 2: the sensor radius lies beyond the exit-pupil LUT's last key
        if self.model == RAYTRACED and self.last_lut_key is not None:
            past = live & (np.hypot(ps[:, 0], ps[:, 1]) * self.half_sensor > self.last_lut_key)
        return dict(ps=ps, traced=live, reason=reason, iface=iface, clear=clear, clearance=clearance, cap=cap, other=other, past_lut=past)

    def edge(self, res, stop_band=1e-2, band=1e-4):
        """the rays whose clip decision rounding may take: |clearance| below stop_band at the stop, below band at any other interface
        (the thin lens: below band at its one limit)"""
        c = np.abs(res["clear"])
        lim = np.full(c.shape[1], band)
        if self.model == RAYTRACED:
            lim[self.stop] = stop_band
        with np.errstate(invalid="ignore"):
            return (c < lim[None, :]).any(1)

    def decision_edge(self, res, stop_band=1e-2, band=1e-4, cap_band=1e-5):
        """edge(), and the rays whose sphere-miss or total-reflection margin is below band, or whose start point lies within cap_band
        (in front housing radii) of the limit behind the front cap: the set to leave out where the REASON a ray ended is compared.
        (cap_band: the start point and the cap are f32 numbers of the size of that radius, good to ~1e-7 of it; a forward record's own
        start point lies ON the cap, 6e-5 from the limit, and must stay in the set.)"""
        with np.errstate(invalid="ignore"):
            return self.edge(res, stop_band, band) | (np.abs(res["other"]) < band).any(1) | (np.abs(res["cap"] + CAP_SLACK) < cap_band)

"""numpy restatement of the ghost tracer (zoic_amd/csrc/ghost.hpp) for the tests, in f64 and in plain sphere geometry: absolute
coordinates, every interface a sphere about its centre (vertex - R, the vertices being the prescription's running f32 thickness sums
that the library's tables hold), the classic tca / thc intersection.  It shares no operation order with the f32 vertex form.

A ghost is defined for a start (o, d) in the forward trace's frame, a wavelength and a pair (a, b), a > b, trace-order indices; the
pair (-1, -1) is the plain refracting path.  lens(info) gathers the geometry of a ZoicCamera.info(); ghost(...) traces n starts through
one pair and returns, per ghost, the record (origin, dir, weight), the reason / interface / leg where it ended, and the smallest
relative margin any of its decisions had."""
import numpy as np

import differentials_spectral_ref as sref
import transmittance_ref as tref

F32 = np.float32
TRACED, MISS, CLIPPED, TIR, TURNED, NO_REFLECTION, NON_FINITE, WAVELENGTH, NO_START, MODEL, INVALID_PAIR = range(11)
MARGIN = 1e-4          # a ghost whose f64 path came closer than this (relative) to any decision may be left out ...
MAX_LEFT_OUT = 0.02    # ... and at most this share of a lens's ghosts is
REASONS = ("traced", "miss", "clipped", "tir", "turned", "no reflection", "non-finite", "wavelength", "no start", "model", "invalid pair")


def bound(measured):
    """what is asserted for a table of measured errors: 4 x them, the project's margin for other compilers' host builds"""
    return {k: 4 * v for k, v in measured.items()}


def expected_pairs(disp):
    """the pair list of a lens by the d-line rule: (a, b), a > b, both interfaces between differing media"""
    n1 = disp["ior_d"]
    differ = n1 != np.append(n1[1:], F32(1.0))
    return np.array([(a, b) for a in range(len(n1)) for b in range(a) if differ[a] and differ[b]], np.int32).reshape(-1, 2)


def flag_word(reason, interface=0, leg=0):
    """the record's flag word: bit 0 for a traced ghost, else reason << 8 | interface << 16 | leg << 24"""
    reason, interface, leg = (np.asarray(v, np.uint32) for v in (reason, interface, leg))
    return np.where(reason == TRACED, np.uint32(1), (reason << np.uint32(8)) | (interface << np.uint32(16)) | (leg << np.uint32(24)))


def lens(info):
    """the geometry of ZoicCamera.info(): dict of count, radius, vertex (f32 running sum of the thicknesses, computeLensCenters),
    housing2 (Surface::housing2: the largest f32 <= (aperture / 2)^2, at the stop also <= userApertureRadius^2), and the rows the host
    driver fills its table from"""
    n = int(info["lensCount"])
    el = info["elements"][:n]
    radius, thickness, aperture = el[:, 0].astype(F32), el[:, 1].astype(F32), el[:, 3].astype(F32)
    vtx = np.zeros(n, F32)
    s = F32(0)
    for i in range(n):
        s = thickness[0] if i == 0 else F32(s + thickness[i])
        vtx[i] = s
    want = (aperture.astype(np.float64) * 0.5) ** 2
    h = want.astype(F32)
    over = h.astype(np.float64) > want
    h[over] = np.nextafter(h[over], F32(-np.inf))
    stop = int(info["apertureElement"])
    user = F32(info["userApertureRadius"])
    h[stop] = min(h[stop], F32(user * user))
    return dict(count=n, radius=radius, thickness=thickness, aperture=aperture, vertex=vtx, housing2=h, stop=stop, user=user)


def sequence(count, a, b):
    """the interface visits of the pair: (leg, interface, reflect) in order"""
    if a == -1 and b == -1:
        return [(0, i, False) for i in range(count)]
    seq = [(0, i, False) for i in range(a)] + [(0, a, True)]
    seq += [(1, i, False) for i in range(a - 1, b, -1)] + [(1, b, True)]
    return seq + [(2, i, False) for i in range(b + 1, count)]


def ghost(L, disp, lam, o, d, a, b, film_index=None, film_lambda0=None, have_start=None, model=1):
    """n ghosts of the pair (a, b) from the starts (o, d) (n,3) at the wavelengths lam (n,).  L = lens(info), disp the camera's dispersion
    table, the film arrays in trace order (None: uncoated), have_start (n,) bool (None: all).  Returns a dict of origin (n,3), dir (n,3),
    weight (n,) -- zeros for a ghost that ended early --, reason, interface, leg (n,) and margin (n,): the smallest of
    |h^2 - housing2| / housing2, |R^2 - d2| / R^2 (the vertex form's discriminant), |k2| and |u.z| over the decisions the ghost met,
    the one that ended it included (inf for a ghost that met none)."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    lam32 = np.asarray(lam, F32)
    lam = lam32.astype(np.float64)
    n, count = len(o), L["count"]
    reason = np.zeros(n, np.int64)
    iface = np.zeros(n, np.int64)
    legs = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    alive = np.ones(n, bool)

    def end(mask, why, i=0, leg=0):
        mask = mask & alive
        reason[mask], iface[mask], legs[mask] = why, i, leg
        alive[mask] = False

    every = np.ones(n, bool)
    plain = a == -1 and b == -1
    if model != 1:
        end(every, MODEL)
    if not plain and not (0 <= b < a < count):
        end(every, INVALID_PAIR)
    if have_start is not None:
        end(~np.asarray(have_start, bool), NO_START)
    end(~((lam32 >= F32(360)) & (lam32 <= F32(830))), WAVELENGTH)
    out = dict(origin=np.zeros((n, 3)), dir=np.zeros((n, 3)), weight=np.zeros(n), reason=reason, interface=iface, leg=legs, margin=margin)
    if not alive.any():
        return out
    with np.errstate(all="ignore"):
        safe = np.where(np.isfinite(lam) & (lam > 0), lam, 500.0)
        index = np.concatenate([sref.cauchy_index(disp, safe), np.ones((n, 1))], 1)    # index[:, i] behind interface i; 1.0 in front
        if not plain:
            end(index[:, a] == index[:, a + 1], NO_REFLECTION, a, 0)
            end(index[:, b] == index[:, b + 1], NO_REFLECTION, b, 1)
        finite = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).max(1) > 0)
        end(~finite, NON_FINITE)
        nc = np.zeros(count) if film_index is None else np.asarray(film_index, np.float64)
        l0 = np.zeros(count) if film_lambda0 is None else np.asarray(film_lambda0, np.float64)
        p = o.copy()
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
        w = np.ones(n)

        def decide(value, fails, why, i, leg):
            margin[alive] = np.minimum(margin[alive], np.abs(value[alive]))
            end(fails, why, i, leg)

        leg = 0
        for leg, i, reflect in sequence(count, a, b) if alive.any() else []:
            sgn = -1.0 if leg == 1 else 1.0                                  # the leg's direction along z
            R = float(L["radius"][i])
            C = np.array([0.0, 0.0, float(L["vertex"][i]) - R])
            decide(u[:, 2], ~(u[:, 2] * sgn > 0), TURNED, i, leg)
            Lv = C[None, :] - p
            tca = (Lv * u).sum(1)
            d2 = (Lv * Lv).sum(1) - tca * tca
            disc = (R * R - d2) / (R * R)
            decide(disc, ~(disc >= 0), MISS, i, leg)
            thc = np.sqrt(np.abs(R * R - d2))
            t = tca + thc * np.sign(R) * sgn                                 # the vertex-side hit (zoic.cpp:986 for a +z ray)
            hit = p + u * t[:, None]
            h2 = hit[:, 0] ** 2 + hit[:, 1] ** 2
            H = float(L["housing2"][i])
            decide((h2 - H) / H, ~(h2 <= H), CLIPPED, i, leg)
            N = (hit - C[None, :]) / R * -sgn                                # towards where the leg comes from
            cosi = -(u * N).sum(1)
            n_from, n_to = (index[:, i], index[:, i + 1]) if leg != 1 else (index[:, i + 1], index[:, i])
            eta = n_from / n_to
            k2 = 1.0 - eta * eta * (1.0 - cosi * cosi)
            ct = np.sqrt(np.abs(k2))
            T = tref.interface_transmittance(n_from, n_to, np.abs(cosi), ct, nc[i], l0[i], safe)
            if reflect:
                margin[alive] = np.minimum(margin[alive], np.abs(k2[alive]))
                w = w * np.where(k2 >= 0, 1.0 - T, 1.0)
                u = u + 2.0 * cosi[:, None] * N
            else:
                decide(k2, ~(k2 >= 0), TIR, i, leg)
                w = w * T
                u = eta[:, None] * u + (eta * cosi - ct)[:, None] * N
            p = hit
        decide(u[:, 2], ~(u[:, 2] > 0), TURNED, count - 1, leg)
        end(~(np.isfinite(p).all(1) & np.isfinite(u).all(1) & np.isfinite(w)), NON_FINITE, count - 1, leg)
    out["origin"][alive] = -p[alive]
    out["dir"][alive] = -u[alive]
    out["weight"][alive] = w[alive]
    return out


def paraxial(L, index, a, b, y0, s0):
    """(height, slope) at the front vertex of the paraxial ray that starts at height y0 with slope s0 = dy/dz in the plane of the rear
    vertex: the product of the refraction, transfer and reflection matrices of the pair's three legs.  index: count + 1 indices, [i]
    behind interface i, 1.0 in front.  Slopes are dy/dz in the fixed frame, whichever way the ray travels."""
    y, s = float(y0), float(s0)
    z = float(L["vertex"][0])
    for leg, i, reflect in sequence(L["count"], a, b):
        zv = float(L["vertex"][i])
        y, z = y + s * (zv - z), zv
        c = 1.0 / float(L["radius"][i])
        n_from, n_to = (index[i], index[i + 1]) if leg != 1 else (index[i + 1], index[i])
        # the surface is z = vtx - c y^2 / 2 (centre at vtx - R), so its normal is the line of slope dy/dz = c y; Snell's law and the
        # law of reflection on the small angles between the ray's line and that line
        if reflect:
            s = 2.0 * c * y - s
        else:
            s = c * y + (n_from / n_to) * (s - c * y)
    return y, s

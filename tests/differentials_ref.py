"""numpy restatement of the traced ray differentials (zoic_amd/csrc/differentials.hpp) for the tests: the f64 trace of ONE try
through the reference's interfaces (zoic.cpp:973-1025, the function the library evaluates), its central differences with the
lens point L held fixed, and the replay of a ray's accepted try (the lens point) from the oracle's own helpers."""
import ctypes as C

import numpy as np

F32 = np.float32
COS_MIN = 0.05      # the conditioning rule: a ray whose min_cos_incidence is below it has no reliable finite difference


def surfaces(info):
    """interface table of ZoicCamera.info() / OracleCamera.lens_table(): (center, radius2, sign, eta) as float32 columns,
    the values csrc/lens_system.cpp fill_surfaces derives"""
    el = info["elements"]
    n = int(info["lensCount"])
    r, ior, center = el[:n, 0].astype(F32), el[:n, 2].astype(F32), el[:n, 4].astype(F32)
    nxt = np.append(ior[1:], F32(1.0)).astype(F32)
    eta = np.where(nxt == F32(1.0), ior, (ior / nxt).astype(F32)).astype(F32)
    return np.stack([center, (r * r).astype(F32), np.where(r < 0, F32(-1), F32(1)), eta], 1).astype(F32)


def _interface(o, d, c, r2, sg, eta):
    """one interface of the f64 trace: (hit point, refracted direction, cos of the incidence angle, cos of the refraction angle)"""
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    L = np.stack([-o[:, 0], -o[:, 1], c - o[:, 2]], 1)
    tca = (L * u).sum(1)
    d2 = (L * L).sum(1) - tca * tca
    thc = np.sqrt(np.abs(r2 - d2))
    t = tca + thc * sg
    hit = o + u * t[:, None]
    cv = np.stack([-hit[:, 0], -hit[:, 1], c - hit[:, 2]], 1)
    N = cv / np.linalg.norm(cv, axis=1, keepdims=True) * sg
    c1 = -(u * N).sum(1)
    cs2 = eta * eta * (1.0 - c1 * c1)
    ct = np.sqrt(np.abs(1.0 - cs2))
    k = eta * c1 - ct
    return hit, u * eta + N * k[:, None], c1, ct


def trace(surf, o, d):
    """f64 trace of (n,3) origins / directions through every interface (no clip: the rays are known to pass); returns the
    traced (o, d) BEFORE the final flip"""
    o = np.asarray(o, np.float64).copy()
    d = np.asarray(d, np.float64).copy()
    for c, r2, sg, eta in np.asarray(surf, np.float64):
        o, d, _, _ = _interface(o, d, c, r2, sg, eta)
    return o, d


def kolb_jacobian_fd(surf, half_sensor, o0, d0, h=1e-5):
    """(n,12) central differences of the flipped (O, D) w.r.t. sx and sy with L = o0.xy + d0.xy fixed: columns dOdx, dOdy, dDdx, dDdy"""
    o0 = np.asarray(o0, np.float64)
    d0 = np.asarray(d0, np.float64)
    cols = {}
    for axis, name in ((0, "x"), (1, "y")):
        step = np.zeros(3)
        step[axis] = h * float(half_sensor)
        op, dp = trace(surf, o0 + step, d0 - step)
        om, dm = trace(surf, o0 - step, d0 + step)
        cols["dO" + name] = -(op - om) / (2 * h)
        cols["dD" + name] = -(dp - dm) / (2 * h)
    return np.concatenate([cols["dOx"], cols["dOy"], cols["dDx"], cols["dDy"]], 1)


def thin_jacobian_fd(sx, sy, tan_fov, origin, focal_distance, dof, h=1e-5):
    """(n,12) central differences of the flipped thin-lens direction normalize(p |fd| - origin) (dof) or normalize(p); dO = 0"""
    sx = np.asarray(sx, np.float64)
    sy = np.asarray(sy, np.float64)
    origin = np.asarray(origin, np.float64)

    def D(x, y):
        p = np.stack([x * tan_fov, y * tan_fov, np.ones_like(x)], 1)
        q = p * abs(focal_distance) - origin if dof else p
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        q[:, 2] *= -1.0
        return q
    ddx = (D(sx + h, sy) - D(sx - h, sy)) / (2 * h)
    ddy = (D(sx, sy + h) - D(sx, sy - h)) / (2 * h)
    z = np.zeros_like(ddx)
    return np.concatenate([z, z, ddx, ddy], 1)


def rel_err(got, ref, floor=1e-12):
    """per 3-vector relative error |got - ref| / |ref| of (n,12) arrays -> (n,4)"""
    g = np.asarray(got, np.float64).reshape(-1, 4, 3)
    r = np.asarray(ref, np.float64).reshape(-1, 4, 3)
    return np.linalg.norm(g - r, axis=2) / np.maximum(np.linalg.norm(r, axis=2), floor)


# ---- replay of the accepted try (what csrc/differentials.hip rebuilds on the device), from the oracle's helpers ----------
def accepted_draws(samples, tries, states, oracle_lib):
    """(u, v) of each ray's accepted try: (lensx, lensy) for try 0, else draws 2a-1 and 2a of its xorshift128 stream"""
    L = oracle_lib.lib()
    n = len(tries)
    u = samples[:, 2].astype(F32).copy()
    v = samples[:, 3].astype(F32).copy()
    for i in np.nonzero(tries > 0)[0]:
        r = oracle_lib.Rng(*[int(x) for x in states[i]])
        for _ in range(2 * int(tries[i]) - 2):
            L.zo_xor128(C.byref(r))
        a = L.zo_xor128(C.byref(r))
        b = L.zo_xor128(C.byref(r))
        u[i] = F32(a / 4294967296.0)
        v[i] = F32(b / 4294967296.0)
    assert len(u) == n
    return u, v


def lens_samples(oc, u, v, image):
    """the oracle's lens sampler (concentric disk or bokeh image), one ray at a time"""
    L = oc._L
    out = np.zeros((len(u), 2), F32)
    if image:
        x, y = C.c_float(), C.c_float()
        for i in range(len(u)):
            L.zo_bokeh_sample(oc._h, float(u[i]), float(v[i]), C.byref(x), C.byref(y))
            out[i] = (x.value, y.value)
    else:
        p = L.zo_concentric_disk_sample.argtypes[2]._type_()
        for i in range(len(u)):
            L.zo_concentric_disk_sample(float(u[i]), float(v[i]), C.byref(p))
            out[i] = (p.x, p.y)
    return out


def kolb_start(oc, params, samples, tries, states, oracle_lib):
    """(o0, d0) of each ray's accepted try, f32 as the reference computes them (zoic.cpp:1853-1943)"""
    lt = oc.lens_table()
    el = lt["elements"]
    hs = F32(F32(params["sensorWidth"]) * F32(0.5))
    o0 = np.stack([samples[:, 0] * hs, samples[:, 1] * hs, np.full(len(samples), lt["originShift"], F32)], 1).astype(F32)
    u, v = accepted_draws(samples, tries, states, oracle_lib)
    lens = lens_samples(oc, u, v, bool(params.get("useImage")))
    if not params.get("kolbSamplingLUT", True):
        Lxy = (lens * el[0, 3]).astype(F32)
    else:
        keys, boxes = oc.lut()
        cx = ((boxes[:, 2] + boxes[:, 0]) * F32(0.5)).astype(F32)
        cy = ((boxes[:, 3] + boxes[:, 1]) * F32(0.5)).astype(F32)
        scale = np.maximum(np.abs(boxes[:, 0] - cx), np.abs(boxes[:, 1] - cy)).astype(F32)
        dist = np.abs(np.sqrt((o0[:, 0] * o0[:, 0] + o0[:, 1] * o0[:, 1]).astype(F32))).astype(F32)
        low = np.searchsorted(keys, dist, side="left")
        inside = dist <= keys[-1]
        lo = np.clip(low, 1, len(keys) - 1)
        pct = ((dist - keys[lo]) / (keys[lo - 1] - keys[lo])).astype(F32)
        ms = ((scale[lo] + pct * (scale[lo - 1] - scale[lo])) * F32(1.05)).astype(F32)
        tr = (cx[lo] + pct * (cx[lo - 1] - cx[lo])).astype(F32)
        ms = np.where(low == 0, scale[0] * F32(1.05), ms)
        tr = np.where(low == 0, cx[0], tr)
        ms = np.where(inside, ms, F32(0)).astype(F32)
        tr = np.where(inside, tr, F32(0)).astype(F32)
        theta = np.arctan2(o0[:, 1].astype(np.float64), o0[:, 0].astype(np.float64)).astype(F32)
        L = oc._L
        sn = np.array([L.zo_fast_sin(float(t)) for t in theta], F32)
        cs = np.array([L.zo_fast_cos(float(t)) for t in theta], F32)
        lx = (lens[:, 0] * ms + tr).astype(F32)
        ly = (lens[:, 1] * ms + np.where(tries > 0, tr, F32(0))).astype(F32)
        Lxy = np.stack([lx * cs - ly * sn, lx * sn + ly * cs], 1).astype(F32)
    d0 = np.stack([Lxy[:, 0] - o0[:, 0], Lxy[:, 1] - o0[:, 1], np.full(len(samples), -el[0, 1], F32)], 1).astype(F32)
    return o0, d0


def passing_rays(oc, info, hs, rs, want):
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
    nh = C.c_int()
    for i in range(n):
        oo, dd = oracle.V3(*o[i]), oracle.V3(*d[i])
        if L.zo_trace_record(oc._h, C.byref(oo), C.byref(dd), hits, C.byref(nh)):
            keep.append(i); po.append((oo.x, oo.y, oo.z)); pd.append((dd.x, dd.y, dd.z))
            if len(keep) == want:
                break
    return o[keep], d[keep], np.array(po, np.float64), np.array(pd, np.float64)


def min_cos_incidence(surf, o, d):
    """(n,) smallest |cos i| of each ray's f64 trace (trace's arithmetic) over every interface: the conditioning of its
    Jacobian.  Refraction maps a change of the incidence angle by 1 / cos(t) and the hit point moves by 1 / cos(i) per unit of
    the ray's angle, so a grazing hit anywhere makes the ray's central differences (and its f32 derivatives) unreliable."""
    o = np.asarray(o, np.float64).copy()
    d = np.asarray(d, np.float64).copy()
    worst = np.ones(len(o))
    for c, r2, sg, eta in np.asarray(surf, np.float64):
        o, d, c1, ct = _interface(o, d, c, r2, sg, eta)
        worst = np.minimum(worst, np.minimum(np.abs(c1), ct))
    return worst


def replay_and_restatement(oc, o0, d0, origin, direction):
    """Checks of the start rays kolb_start rebuilt, against the records (origin, direction: (n,3) f32, flipped as stored):
    replay -- (n,) bool: the oracle's own f32 trace (zo_trace_record, traceThroughLensElements) from (o0, d0) gives the record bit
    for bit, i.e. (o0, d0) IS the try the reference traced;  eo, ed -- (n,) relative errors of the f64 restatement (trace) against
    the records.  Where the replay holds and the restatement misses, the gap is the f32 rounding of the reference's own trace."""
    o0 = np.asarray(o0, F32)
    d0 = np.asarray(d0, F32)
    replay = np.zeros(len(o0), bool)
    for i in range(len(o0)):
        ok, _, o, d = oc.trace_record(o0[i], d0[i])
        replay[i] = ok and np.array_equal((o * F32(-1)).view(np.uint32), np.asarray(origin[i], F32).view(np.uint32)) and \
            np.array_equal((d * F32(-1)).view(np.uint32), np.asarray(direction[i], F32).view(np.uint32))
    ro, rd = trace(surfaces(oc.lens_table()), o0, d0)
    eo = np.linalg.norm(-ro - origin, axis=1) / np.linalg.norm(origin, axis=1)
    ed = np.linalg.norm(-rd - direction, axis=1) / np.linalg.norm(direction, axis=1)
    return replay, eo, ed


def restatement_holds(eo, ed):
    """_check_kolb's criterion for the f64 restatement reproducing the records (tests/test_differentials_gpu.py)"""
    return bool(np.median(eo) < 1e-5 and np.median(ed) < 1e-5 and np.percentile(ed, 99.9) < 1e-4)

"""numpy restatement of the traced ray differentials of spectral records (zoic_amd/csrc/differentials_spectral.hpp) for the tests:
differentials_ref's f64 trace of ONE try with an eta per ray and interface, taken from the two-term Cauchy model evaluated in f64 on
the camera's own dispersion table (ZoicCamera.dispersion(): zoic_camera_get_dispersion), and its central differences
  - in the sensor point with the lens point L held fixed (differentials_ref.kolb_jacobian_fd's scheme), and
  - in the wavelength, sensor point and L held fixed (per nanometre).
differentials_ref._interface multiplies the (n,3) unit direction by eta, so it takes one eta for the whole batch; interface() below
is the same arithmetic with an (n,) eta (tests/test_differentials_spectral_cpu.py checks the two against each other bit for bit)."""
import numpy as np

from zoic_amd.camera import ZoicCamera
from zoic_amd.workloads import camera_params

import differentials_ref as dref
from spectral_ref import WAVES

F32 = np.float32
LAMBDA_D, LAMBDA_F, LAMBDA_C = 587.5618, 486.1327, 656.2725   # nm (csrc/spectral.hpp)


def tables(cfg, abbe=None, lens_text=None, **over):
    """(params, info, dispersion, surfaces, halfSensor) of a tables-only camera"""
    p = camera_params(cfg)
    p["useImage"] = False
    p.pop("bokehPath", None)
    p.update(over)
    cam = ZoicCamera(device=-1)
    if lens_text is not None:
        cam.set_lens_text(lens_text)
    cam.update(**p)
    if abbe is not None:
        cam.set_abbe_numbers(np.full(cam.info()["lensCount"], abbe, F32))
    info, disp = cam.info(), cam.dispersion()
    cam.close()
    return p, info, disp, dref.surfaces(info), F32(F32(p["sensorWidth"]) * F32(0.5))


_RAYS = {}


def lens_rays(cfg, oracle_lib, want=10000):
    """~10 k rays the oracle's d-line trace lets through (differentials_ref.passing_rays, seed 11), computed once per lens and shared
    by the CPU tests of the spectral differentials, the transmittance and the ghosts: not to be written to"""
    if cfg not in _RAYS:
        p, info, _, _, hs = tables(cfg)
        oc = oracle_lib.OracleCamera()
        oc.update(**p)
        o, d, _, _ = dref.passing_rays(oc, info, hs, np.random.RandomState(11), want)
        assert len(o) >= want // 2, (cfg, len(o))
        o.setflags(write=False)
        d.setflags(write=False)
        _RAYS[cfg] = (o, d)
    return _RAYS[cfg]


def ray_wavelengths(n, seed=4):
    lam = np.random.RandomState(seed).uniform(400, 700, n).astype(F32)
    lam[:8 * (n // 64):n // 64][:8] = WAVES   # the eight fixed ones, spread over the batch
    return lam


def passes(surf, eta, o, d, aperture=None):
    """the f64 trace meets every sphere and refracts everywhere (no |.| of the restatement flips a sign): the path is a real one;
    aperture (count,): the hit points also lie within each interface's housing"""
    o = np.asarray(o, np.float64).copy()
    d = np.asarray(d, np.float64).copy()
    ok = np.ones(len(o), bool)
    for i, (c, r2, sg, _) in enumerate(np.asarray(surf, np.float64)):
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
        L = np.stack([-o[:, 0], -o[:, 1], c - o[:, 2]], 1)
        tca = (L * u).sum(1)
        ok &= (L * L).sum(1) - tca * tca <= r2
        o, d, c1, _ = interface(o, d, c, r2, sg, eta[:, i])
        ok &= eta[:, i] ** 2 * (1 - c1 * c1) <= 1.0
        if aperture is not None:
            ok &= o[:, 0] ** 2 + o[:, 1] ** 2 <= (0.5 * float(aperture[i])) ** 2
    return ok


def cauchy_index(disp, lam):
    """(n, count) f64 indices n_i(lambda) = n_d,i + B_i (1/lambda^2 - 1/lambda_d^2) of the media behind each interface (trace order)"""
    lam = np.asarray(lam, np.float64).reshape(-1, 1)
    nd = np.asarray(disp["ior_d"], np.float64)[None, :]
    b = np.asarray(disp["cauchy_b"], np.float64)[None, :]
    return nd + b * (1.0 / (lam * lam) - 1.0 / (LAMBDA_D * LAMBDA_D))


def cauchy_eta(disp, lam):
    """(n, count) f64 eta_i = n_i / n_i+1, n = 1 behind the last interface (zoic.cpp:1013 and :1137-1143)"""
    n = cauchy_index(disp, lam)
    nxt = np.concatenate([n[:, 1:], np.ones((len(n), 1))], 1)
    return n / nxt


def interface(o, d, c, r2, sg, eta):
    """differentials_ref._interface with an (n,) eta: (hit point, refracted direction, cos i, cos t)"""
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
    return hit, u * np.reshape(eta, (-1, 1)) + N * k[:, None], c1, ct


def trace(surf, eta, o, d):
    """f64 trace of (n,3) origins / directions through every interface with eta (n, count); (o, d) BEFORE the final flip, and the
    smallest |cos i|, cos t and the largest (d2 - radius2) met (a ray that passes has the last one <= 0)"""
    o = np.asarray(o, np.float64).copy()
    d = np.asarray(d, np.float64).copy()
    worst = np.ones(len(o))
    for i, (c, r2, sg, _) in enumerate(np.asarray(surf, np.float64)):
        o, d, c1, ct = interface(o, d, c, r2, sg, eta[:, i])
        worst = np.minimum(worst, np.minimum(np.abs(c1), ct))
    return o, d, worst


def min_cos_incidence(surf, eta, o, d):
    """differentials_ref.min_cos_incidence with eta (n, count): (n,) smallest |cos i| / cos t of each ray's f64 trace at its own
    wavelength, the conditioning of its Jacobian (trace's own arithmetic: the third thing it returns)"""
    return trace(surf, eta, o, d)[2]


def jacobian_fd(surf, disp, lam, half_sensor, o0, d0, h=1e-5):
    """(n,12) central differences of the flipped (O, D) w.r.t. sx and sy with L = o0.xy + d0.xy fixed, at each ray's wavelength:
    columns dOdx, dOdy, dDdx, dDdy"""
    o0 = np.asarray(o0, np.float64)
    d0 = np.asarray(d0, np.float64)
    eta = cauchy_eta(disp, lam)
    cols = {}
    for axis, name in ((0, "x"), (1, "y")):
        step = np.zeros(3)
        step[axis] = h * float(half_sensor)
        op, dp, _ = trace(surf, eta, o0 + step, d0 - step)
        om, dm, _ = trace(surf, eta, o0 - step, d0 + step)
        cols["dO" + name] = -(op - om) / (2 * h)
        cols["dD" + name] = -(dp - dm) / (2 * h)
    return np.concatenate([cols["dOx"], cols["dOy"], cols["dDx"], cols["dDy"]], 1)


def wavelength_fd(surf, disp, lam, o0, d0, h=0.05):
    """(n,6) central differences of the flipped (O, D) w.r.t. the wavelength (per nm), sensor point and L fixed: dO/dlambda, dD/dlambda"""
    lam = np.asarray(lam, np.float64)
    op, dp, _ = trace(surf, cauchy_eta(disp, lam + h), o0, d0)
    om, dm, _ = trace(surf, cauchy_eta(disp, lam - h), o0, d0)
    return np.concatenate([-(op - om) / (2 * h), -(dp - dm) / (2 * h)], 1)


def rel_err_floor(got, ref, floor_share=1e-3):
    """per 3-vector |got - ref| / max(|ref|, floor) of (n, 3m) arrays -> (n, m); floor = floor_share x the batch's median |ref| per
    vector, so that rays whose tangent vanishes (near the axis) do not set the figure"""
    g = np.asarray(got, np.float64).reshape(len(got), -1, 3)
    r = np.asarray(ref, np.float64).reshape(len(ref), -1, 3)
    mag = np.linalg.norm(r, axis=2)
    floor = floor_share * np.median(mag, axis=0, keepdims=True)
    return np.linalg.norm(g - r, axis=2) / np.maximum(mag, floor)


def wavelength_contributions(surf, disp, lam, o0, d0, h=0.05):
    """(n,2) sum over the interfaces of |the wavelength tangent that interface's eta alone contributes| (dO, dD): central differences
    with one column of eta moved at a time.  On an achromatised lens the contributions of crown and flint cancel in their sum, the
    tangent itself, which f32 arithmetic therefore holds to its rounding TIMES sum / |tangent|."""
    lam = np.asarray(lam, np.float64)
    e0, ep, em = cauchy_eta(disp, lam), cauchy_eta(disp, lam + h), cauchy_eta(disp, lam - h)
    total = np.zeros((len(lam), 2))
    for i in range(e0.shape[1]):
        a, b = e0.copy(), e0.copy()
        a[:, i], b[:, i] = ep[:, i], em[:, i]
        op, dp, _ = trace(surf, a, o0, d0)
        om, dm, _ = trace(surf, b, o0, d0)
        total[:, 0] += np.linalg.norm(op - om, axis=1) / (2 * h)
        total[:, 1] += np.linalg.norm(dp - dm, axis=1) / (2 * h)
    return total

"""numpy restatement of the Fresnel transmittance of a traced ray (zoic_amd/csrc/transmittance.hpp) for the tests, in f64:
differentials_spectral_ref.interface's trace of ONE try -- it already returns cos i and cos t at every interface -- with the Cauchy
indices of the camera's own dispersion table (ZoicCamera.dispersion()) and the film arrays of ZoicCamera.coatings() (trace order;
index 0: uncoated), and at every interface the transmittance of unpolarised light, bare or through a quarter-wave film."""
import os

import numpy as np

from zoic_amd.camera import LENS_DIR, ZoicError

import differentials_spectral_ref as sref

F32 = np.float32
FILM_INDEX, FILM_LAMBDA0 = F32(1.38), F32(550.0)     # MgF2, a quarter wave thick in the green


def housings(info):
    """Surface::housing2 of every interface (csrc/lens_system.cpp fill_surfaces): the largest f32 <= (aperture / 2)^2 in f64; the
    stop's is the smaller of that and userApertureRadius^2 in f32"""
    a = info["elements"][:int(info["lensCount"]), 3].astype(np.float64)
    want = (a * 0.5) ** 2
    h = want.astype(F32)
    over = h.astype(np.float64) > want
    h[over] = np.nextafter(h[over], F32(-np.inf))
    stop = int(info["apertureElement"])
    h[stop] = min(h[stop], F32(info["userApertureRadius"]) * F32(info["userApertureRadius"]))
    return h


def films_where_media_differ(disp):
    """(index, lambda0) in trace order: FILM_INDEX / FILM_LAMBDA0 on every interface whose two media differ at the d-line"""
    n1 = disp["ior_d"]
    differ = n1 != np.append(n1[1:], F32(1.0))
    return np.where(differ, FILM_INDEX, F32(0)).astype(F32), np.where(differ, FILM_LAMBDA0, F32(0)).astype(F32)


def _loads(lens):
    try:
        sref.tables("C2", lensDataPath=os.path.join(LENS_DIR, lens))
        return True
    except ZoicError as e:      # two of the shipped files list no stop: ZOIC_ERR_NO_APERTURE, no camera to trace through
        assert e.status_name == "ZOIC_ERR_NO_APERTURE", (lens, e)
        return False


# the shipped prescriptions a camera loads
LENSES = [f for f in sorted(os.listdir(LENS_DIR)) if f.endswith(".dat") and _loads(f)]
assert len(LENSES) >= 6 and {"tessar_f2.8.dat", "double_gauss_f2.0.dat", "petzval_f1.25.dat"} <= set(LENSES)


def uncoated(n1, n2, ci, ct):
    """T_i = 1 - (rs^2 + rp^2) / 2 of a bare interface n1 -> n2 met at cos i = ci, leaving at cos t = ct"""
    rs = (n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)
    rp = (n1 * ct - n2 * ci) / (n1 * ct + n2 * ci)
    return 1.0 - (rs * rs + rp * rp) / 2.0


def _airy(a, b, c2b):
    return (a * a + b * b + 2.0 * a * b * c2b) / (1.0 + a * a * b * b + 2.0 * a * b * c2b)


def coated(n1, n2, ci, ct, nc, lambda0, lam):
    """T_i of the interface under a film of index nc, a quarter wave thick at lambda0; where the film carries no wave (evanescent) the
    bare interface's"""
    s2 = (n1 / nc) ** 2 * (1.0 - ci * ci)
    cc = np.sqrt(np.clip(1.0 - s2, 0.0, None))
    c2b = np.cos(np.pi * (lambda0 / lam) * cc)
    a_s, b_s = (n1 * ci - nc * cc) / (n1 * ci + nc * cc), (nc * cc - n2 * ct) / (nc * cc + n2 * ct)
    a_p, b_p = (n1 * cc - nc * ci) / (n1 * cc + nc * ci), (nc * ct - n2 * cc) / (nc * ct + n2 * cc)
    with_film = 1.0 - (_airy(a_s, b_s, c2b) + _airy(a_p, b_p, c2b)) / 2.0
    return np.where(s2 > 1.0, uncoated(n1, n2, ci, ct), with_film)


def interface_transmittance(n1, n2, ci, ct, nc, lambda0, lam):
    """T_i with the rules of transmittance.hpp: 1 between equal media whatever the film; nc == 0: uncoated"""
    n1, n2, ci, ct, lam = (np.asarray(a, np.float64) for a in np.broadcast_arrays(n1, n2, ci, ct, lam))
    t = uncoated(n1, n2, ci, ct) if nc == 0 else coated(n1, n2, ci, ct, float(nc), float(lambda0), lam)
    return np.where(n1 == n2, 1.0, t)


def transmittance(surf, disp, lam, o, d, film_index=None, film_lambda0=None):
    """(T (n,), passes (n,)) of the tries (o, d) (n,3) at wavelengths lam (n,): surf = differentials_ref.surfaces(info), disp the
    camera's dispersion table, the film arrays in trace order (None: uncoated).  passes: the f64 path meets every sphere and is
    nowhere totally reflected (housings are not looked at); T is meaningless elsewhere."""
    lam = np.asarray(lam, np.float64)
    index = sref.cauchy_index(disp, lam)
    nxt = np.concatenate([index[:, 1:], np.ones((len(index), 1))], 1)
    eta = index / nxt
    count = len(surf)
    nc = np.zeros(count) if film_index is None else np.asarray(film_index, np.float64)
    l0 = np.zeros(count) if film_lambda0 is None else np.asarray(film_lambda0, np.float64)
    o = np.asarray(o, np.float64).copy()
    d = np.asarray(d, np.float64).copy()
    T = np.ones(len(o))
    ok = np.ones(len(o), bool)
    for i, (c, r2, sg, _) in enumerate(np.asarray(surf, np.float64)):
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
        L = np.stack([-o[:, 0], -o[:, 1], c - o[:, 2]], 1)
        tca = (L * u).sum(1)
        ok &= (L * L).sum(1) - tca * tca <= r2
        o, d, c1, ct = sref.interface(o, d, c, r2, sg, eta[:, i])
        ok &= ~((index[:, i] > nxt[:, i]) & (eta[:, i] ** 2 * (1.0 - c1 * c1) > 1.0))
        T = T * interface_transmittance(index[:, i], nxt[:, i], np.abs(c1), ct, nc[i], l0[i], lam)
    return T, ok


def on_axis_closed_form(ior_d):
    """prod_i 1 - ((n1 - n2) / (n1 + n2))^2 over a prescription's interfaces (trace order, air behind the last): a bare lens met along
    its axis"""
    n1 = np.asarray(ior_d, np.float64)
    n2 = np.append(n1[1:], 1.0)
    return float(np.prod(1.0 - ((n1 - n2) / (n1 + n2)) ** 2))

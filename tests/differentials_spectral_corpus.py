"""What the corpus tests of the spectral ray differentials share (tests/test_differentials_spectral_corpus_cpu.py and its GPU twin), and
what the transmittance and ghost corpus tests take from them: the frame traceback_cases.frame_samples() with one wavelength per ray,
uniform in [400, 700] nm with the eight spectral_ref.WAVES spread over it (frame); which of a lens's live rows get the f64 reference, at
most 4 096 (reference_rows); the reference itself (reference: surfaces from differentials_ref.surfaces, eta per ray and interface from
sref.cauchy_eta on the camera's dispersion(), sref.jacobian_fd, sref.wavelength_fd at two steps, sref.wavelength_contributions); the
conditioning rule and the figures (conditions, figures); the groups of lenses (ACCURACY, IDENTITIES_ONLY, HOST_DEVICE).  A helper, not a
test."""
import numpy as np

import differentials_ref as dref
import differentials_spectral_ref as sref
import machine_lens_corpus as mc
import traceback_cases as tc
from differentials_ref import COS_MIN
from spectral_ref import WAVES

F32 = np.float32
MAX_FD = 4096                      # rays of a lens that get the f64 finite differences
WAVE_PERIOD = 509                  # row i of the frame with i % 509 = k < 8 has the wavelength WAVES[k]
# Lenses held to the exact identities and to the comparison of the kernel with the host build only, with the reason.
IDENTITIES_ONLY = {
    "mori-4": "machine_lens_corpus.BITWISE (a 400 nm projection too close to its bound); 9 retried rays in the frame",
    "rear-9": "machine_lens_corpus.BITWISE: near-hemispherical rear element",
    "rear-12": "machine_lens_corpus.BITWISE: near-hemispherical rear element",
    "petzval-5": "machine_lens_corpus.OUTSIDE: outside the geometric domain",
}
ACCURACY = [n for n in mc.ACCURACY if n not in IDENTITIES_ONLY]
HOST_DEVICE = [n for n in mc.NAMES if n != mc.OUTSIDE]


# ---- the frame ------------------------------------------------------------------------------------------------------------------
_FRAME = []


def frame():
    """(samples (N,4), rng states (N,4), wavelengths (N,) f32) of the corpus frame, cached and not to be written to"""
    if not _FRAME:
        s, st = tc.frame_samples()
        lam = np.random.RandomState(4).uniform(400, 700, tc.N).astype(F32)
        k = np.arange(tc.N) % WAVE_PERIOD
        lam[k < len(WAVES)] = WAVES[k[k < len(WAVES)]]   # the eight fixed ones, each on every 509th row: all over the frame and the wave
        _FRAME.extend([s, st, lam])
        for a in _FRAME:
            a.setflags(write=False)
    return tuple(_FRAME)


def reference_rows(live_rows, tries):
    """the rows of the frame that get the f64 reference, at most MAX_FD: the live rows that carry one of the eight WAVES, a stride of
    the live rows accepted at a retry (tries (N,) > 0; a quarter of MAX_FD at most) and a stride of all live rows"""
    live_rows = np.asarray(live_rows)
    fixed = live_rows[live_rows % WAVE_PERIOD < len(WAVES)]
    retried = mc.strided(live_rows[tries[live_rows] > 0], MAX_FD // 4)
    return np.unique(np.concatenate([mc.strided(live_rows, MAX_FD - len(fixed) - len(retried)), retried, fixed]))


def wave_with(live, least, after=4):
    """the first wave (64 consecutive rows) after wave `after` with at least `least` live rows"""
    per = live[:len(live) // 64 * 64].reshape(-1, 64).sum(1)
    return int(np.flatnonzero(per[after + 1:] >= least)[0]) + after + 1


_TABLES = {}


def tables(name):
    """(params, info, dispersion, halfSensor) of a tables-only camera behind a corpus lens, cached and not to be written to"""
    if name not in _TABLES:
        cam, p = mc.camera(name)
        _TABLES[name] = p, cam.info(), cam.dispersion(), F32(F32(p["sensorWidth"]) * F32(0.5))
        cam.close()
        for table in _TABLES[name][1:3]:
            for a in table.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _TABLES[name]


def reference(surf, disp, hs, lam, o0, d0):
    """The f64 reference of the start rays (o0, d0) at the wavelengths lam: cos (n,) the smallest |cos| met, fd (n,12) the screen
    tangents, wfd (n,6) the wavelength tangent (step 0.05 nm), wfd_half the same at half the step, part (n,2) the sum of the
    interfaces' contributions, end (o, d) the traced ray before the flip"""
    eta = sref.cauchy_eta(disp, lam)
    ro, rd, cos = sref.trace(surf, eta, o0, d0)
    return dict(cos=cos, end=(ro, rd), fd=sref.jacobian_fd(surf, disp, lam, hs, o0, d0), wfd=sref.wavelength_fd(surf, disp, lam, o0, d0, h=0.05),
                wfd_half=sref.wavelength_fd(surf, disp, lam, o0, d0, h=0.025), part=sref.wavelength_contributions(surf, disp, lam, o0, d0))


def conditions(cos, eo, ed):
    """The reference-only conditions of the accuracy comparison: (good (n,) bool, share excluded, restatement holds on the good rays)"""
    good = cos >= COS_MIN
    return good, float((~good).mean()), bool(good.any() and dref.restatement_holds(eo[good], ed[good]))


def figures(out, chroma, ref, good):
    """the figures the accuracy tests assert on, from the library's (n,12) and (n,6) and reference() on the rays `good`"""
    e = dref.rel_err(out[good], ref["fd"][good])
    fd, part = ref["wfd"][good], ref["part"][good]
    el = sref.rel_err_floor(chroma[good], fd)
    ec = np.linalg.norm((chroma[good].astype(np.float64) - fd).reshape(-1, 2, 3), axis=2) / part
    step = sref.rel_err_floor(ref["wfd_half"][good], fd)
    return dict(rays=int(good.sum()), s_med=float(np.median(e)), s_tail=float(np.percentile(e, 99.9)), s_ok=float((e <= 1e-3).mean()),
                c_med=float(np.median(ec)), c_tail=float(np.percentile(ec, 99.9)), l_med=float(np.median(el)),
                l_tail=float(np.percentile(el, 99.9)), step=float(np.percentile(step, 99.9)),
                cancel=float(np.median(part[:, 1] / np.linalg.norm(fd[:, 3:6], axis=1))))


def line(name, m, excluded):
    return "%-10s rays %4d  excluded %.4f  s %.2e / %.2e  c %.2e / %.2e  l %.2e / %.2e  cancellation %.1f" % (
        name, m["rays"], excluded, m["s_med"], m["s_tail"], m["c_med"], m["c_tail"], m["l_med"], m["l_tail"], m["cancel"])

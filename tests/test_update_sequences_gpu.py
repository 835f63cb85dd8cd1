"""The opt-in calls after update sequences and setter changes, on the MI355X: the scripts of tests/update_sequences.py on ONE device
camera and ONE oracle camera per sequence, one test per step (the steps before it are taken first; what a step's checks find is
collected and asserted empty).  tests/test_update_sequences_cpu.py holds every reference-only condition first.

A good RAYTRACED step, n = 2113 samples, the palette of five wavelengths, every device call on the library's OWN streams (rng_states
NULL: the references take ray_rng_states of the step's seed, so the seed is held to at every call):
  tables     info()'s lens arrays and LUT are the oracle's bits; dispersion(), coatings(), ghost_pairs() are the expected tables, again
             after every group of setters applied with no update;
  forward    STRICT: create_rays, create_rays(wavelengths=) and create_rays_hero at k = 4 equal the oracle with the same history, all
             words and the counter deltas (fuzz_cameras._oracle_spectral and hero_ref.hero_reference given that oracle camera).  FAST:
             the flip and RMSE rules of tests/test_hero_reference_gpu.py (fuzz_cameras.FLIP_TOL, DIR_RMSE_TOL) on the same inputs;
  losses     STRICT, after every group: transmittance at k = 1 and k = 4 and the ghosts of up to 32 of the expected pairs equal the
             host builds of csrc/transmittance.hpp and csrc/ghost.hpp from the oracle's recorded starts, every word, under the
             step's dispersion and coatings -- the ghost table the kernel reads is the camera's device copy;
  tangents   STRICT, after every group: the wavelength tangent equals the host build of csrc/differentials_spectral.hpp bit for bit,
             the screen tangents meet the bounds of tests/test_differentials_spectral_corpus_gpu.py against that build and against f64
             (differentials_spectral_corpus.figures, hero_rows.spectral_bounds_hold), the d-line tangents those of
             tests/test_differentials_gpu.py;
  backward   the device batches of projection, trace-back and the Jacobian, d-line and at the palette, equal the host single-item
             calls bit for bit on the step's own forward records, random lines, non-finite rays and a stride of the chief-ray point
             set; the host calls equal a fresh twin's and pass update_sequences.check_backward (host builds from the anchored
             info(), f64 restatements, round trip of the records).
FAST steps run tables, forward and backward.  THINLENS steps: the hero call at k = 4 and n = 65, 2113, 63 (the staging buffer's
first use, its growth, its reuse; two of them on two streams at once) against hero_reference, and the documented dead answers;
NONE: every dead answer.  A failed step: every device call refuses with ZOIC_ERR_NOT_UPDATED and leaves its outputs, prefilled with a
sentinel, alone.

Measured on the MI355X (44 steps, 40 s): no step fails on the library.  E_ref max 1.5e-7 ... 1.1e-6; |library - f64| max 0.35 ... 1.06
E_ref (bound 4), round trip 0.85 ... 1.70 E_ref (bound 5), at the palette 0.71 ... 1.54 of the d-line figure (bound 2); screen tangents
against f64 median 2.1e-7 ... 3.8e-7, 99.9th percentile 1.2e-6 ... 7.5e-6; the FAST step: flip share 0, direction RMSE 4.3e-7.

Would they notice?  The module run once on each of three deliberately wrong libraries (built from copies outside the tree):
  1  fill_backward_tables skipped when the update rebuilt no lens and no image: 5 of 44 red, the THINLENS steps and NONE.  The
     RAYTRACED steps that rebuild nothing stay green, and no test could see it there: nothing the three tables are filled from changes;
  2  the hipMemcpy into dGhost at the first update only: 15 of 44 red (ghosts against the host build, 2.9 K ... 67 K records), every
     RAYTRACED step behind a changed stop limit or lens, while the host calls and the getters stay right;
  3  fill_film and abbe_number answering from a copy taken at the last update: 2 of 44 red, the steps with setters between calls."""
import numpy as np
import pytest

from zoic_amd import PRECISION_STRICT, THINLENS

import device_cases as dc
import differentials_ref as dref
import differentials_spectral_corpus as dsc
import ghost_ref as gref
import hero_ref
import host_drivers
import update_sequences as us
from device_cases import bits
from fuzz_cameras import DIR_RMSE_TOL, FLIP_TOL, _oracle_spectral
from hero_rows import spectral_bounds_hold
from transmittance_ref import housings

pytestmark = pytest.mark.gpu

F32 = np.float32
MAX_PAIRS = 32
_DRIVERS = {}


@pytest.fixture(scope="module", autouse=True)
def _cameras():
    yield
    for D in _DRIVERS.values():
        D.close()
    _DRIVERS.clear()


def _dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _np(t):
    return t.cpu().numpy()


def _words(rays):
    """(..., 8) uint32 of a record tensor"""
    return bits(_np(rays))


def _device_backward(cam, B):
    """the six device batches on update_sequences.backward_inputs B, shaped as update_sequences.host_backward"""
    rec = dc.records(B["o"], B["d"])
    u32 = lambda f: np.ascontiguousarray(f).astype(np.uint32)   # noqa: E731
    tb, tbs = cam.trace_back(rec), cam.trace_back(rec, wavelengths=B["lam"])
    pp, pps = cam.project_points(B["pts"]), cam.project_points(B["pts"], wavelengths=B["plam"])
    j, js = cam.trace_back_jacobian(rec), cam.trace_back_jacobian(rec, wavelengths=B["lam"])
    return {"trace_back": (tb[0], u32(tb[1])), "trace_back_spectral": (tbs[0], u32(tbs[1])), "project": (pp[0], u32(pp[1])),
            "project_spectral": (pps[0], u32(pps[1])), "jacobian": (j[0], u32(j[1]), j[2]), "jacobian_spectral": (js[0], u32(js[1]), js[2])}


def _backward(fail, D, state, info, disp, B, s):
    H = us.host_backward(D.cam, B)
    for line in us.differing(_device_backward(D.cam, B), H):
        fail("the device batch against the host single-item call: " + line)
    us.twin_holds(fail, D, state, D.cam, B, H)
    us.reverse_ray_holds(fail, D.cam, state, B, H)
    return us.check_backward(fail, D.cam, state, info, disp, B, H, s)


def _fast_forward(fail, note, ref, got):
    """tests/test_hero_reference_gpu.py's rule for FAST records against the reference's words"""
    live = ref[:, 0, 6].copy().view(F32) != 0
    rows = (got[:, 0, 7] == ref[:, 0, 7]) & live
    if rows.sum() < 0.95 * live.sum():
        fail("FAST: %d of %d live heroes have the reference's flags" % (rows.sum(), live.sum()))
    a_lost, b_lost = (ref[rows, 1:, 7] & hero_ref.LOST) != 0, (got[rows, 1:, 7] & hero_ref.LOST) != 0
    flip = float((a_lost != b_lost).mean())
    both = ~a_lost & ~b_lost
    da = ref[rows, 1:, 3:6].copy().view(F32)[both].astype(np.float64)
    db = got[rows, 1:, 3:6].copy().view(F32)[both].astype(np.float64)
    finite = np.isfinite(da).all(1)
    rmse = float(np.sqrt(((da[finite] - db[finite]) ** 2).sum(1).mean()))
    h0 = np.sqrt(((ref[rows, 0, 3:6].copy().view(F32).astype(np.float64) - got[rows, 0, 3:6].copy().view(F32)) ** 2).sum(1).mean())
    note["fast"] = dict(rows=int(rows.sum()), flip=flip, rmse=rmse, hero_rmse=float(h0), companions=int(finite.sum()))
    if not (flip < 20 * FLIP_TOL and finite.sum() > 1000 and rmse < DIR_RMSE_TOL and h0 < DIR_RMSE_TOL):
        fail("FAST against the reference: %s" % (note["fast"],))


def _raytraced(D, st, state, note):
    import torch
    fail, cam, oc, p = note["fail"].append, D.cam, D.oc, state.p
    for line in us.anchored(cam, oc, state):
        fail(line)
    bad, disp, film, pairs = us.tables_hold(cam, state)
    for line in bad:
        fail(line)
    info = cam.info()
    s, lam, states = us.inputs(state.seed)
    lam0 = np.ascontiguousarray(lam[:, 0])
    ts, tl, tl0 = _dev(s), _dev(lam), _dev(lam0)
    # ---- the oracle with the same history ------------------------------------------------------------------------------------------
    ref_words, ref_counters, det = hero_ref.hero_reference(D.oracle_lib, p, disp, s, lam, states, details=True, oc=oc)
    ref_spec, ref_spec_counters = _oracle_spectral(D.oracle_lib, p, disp, s, lam0, states, oc=oc)
    before = oc.counters()
    ref_d = oc.create_rays_starts(s, states)
    ref_d_counters = {k: oc.counters()[k] - before[k] for k in before}
    live, starts = ref_words[:, 0, 6].copy().view(F32) != 0, det["starts"]
    note.update(live=int(live.sum()), retried=int((live & (((ref_words[:, 0, 7] >> 1) & 31) > 0)).sum()))
    # ---- forward: the library's own streams of the camera's seed -------------------------------------------------------------------
    hero, hero_counters = dc.delta(cam, lambda: cam.create_rays_hero(ts, tl)["rays"])
    spec, spec_counters = dc.delta(cam, lambda: cam.create_rays(ts, wavelengths=tl0)["rays"])
    plain, plain_counters = dc.delta(cam, lambda: cam.create_rays(ts)["rays"])
    torch.cuda.synchronize()
    hw, sw, pw = _words(hero), _words(spec), _words(plain)
    strict = state.precision == PRECISION_STRICT
    if strict:
        differ = ~hero_ref.same_words(hw, ref_words)
        if differ.any() or hero_counters != ref_counters:
            fail("create_rays_hero: %d records differ from the reference (first %s), counters %s against %s" % (
                differ.sum(), np.argwhere(differ)[:4].tolist(), hero_counters, ref_counters))
        for name, words, counters, ref, rc in (("create_rays(wavelengths=)", sw, spec_counters, ref_spec, ref_spec_counters),
                                               ("create_rays", pw, plain_counters, ref_d, ref_d_counters)):
            want = np.concatenate([bits(ref["planes"]).T, ref["flags"].astype(np.uint32)[:, None]], 1)
            differ = ~hero_ref.same_words(words, want)
            if differ.any() or counters != rc:
                fail("%s: %d records differ from the oracle (first %s), counters %s against %s" % (name, differ.sum(), np.flatnonzero(differ)[:4].tolist(), counters, rc))
    else:
        if info["fastRunsStrict"]:
            fail("the FAST step's camera runs STRICT: it tests nothing")
        _fast_forward(fail, note, ref_words, hw)
        if not np.array_equal(sw, hw[:, 0]):
            fail("FAST: create_rays(wavelengths=) is not column 0 of the hero call")
    # ---- backward ------------------------------------------------------------------------------------------------------------------
    # (the step's own forward records as the ORACLE has them: the STRICT kernel's bits, asserted above; on a FAST step the yardstick
    # E_ref of check_backward is then still the reference's own, not measured on a kernel)
    rec_d, rec_s = np.ascontiguousarray(ref_d["planes"].T), np.ascontiguousarray(det["planes"].T)
    B = us.backward_inputs(info, state, rec_d, rec_s, lam0)
    B["live_d"], B["live_s"] = rec_d[:, 6] != 0, rec_s[:, 6] != 0
    note["backward"] = _backward(fail, D, state, info, disp, B, s)
    if not strict:
        return
    # ---- the passes over the records, under the tables of the update and of every group of setters after it --------------------------
    surf, hs, h2, L = dref.surfaces(info), F32(F32(p["sensorWidth"]) * F32(0.5)), housings(info), gref.lens(info)
    rows = np.flatnonzero(live)
    o0, d0 = starts[rows, 0:3], starts[rows, 3:6]
    through = ref_words[:, :, 6].copy().view(F32) != 0                       # (n, k): the hero and the companions that came through
    ti, tj = np.nonzero(through)
    rows_d = np.flatnonzero(ref_d["weight"] != 0)
    for group in [()] + list(st.between):
        tag = "after %s: " % [g[0] for g in group] if group else ""
        us.apply(cam, state, group)
        bad, disp, film, pairs = us.tables_hold(cam, state)
        for line in bad:
            fail(tag + line)
        coat = film if state.coatings is not None else None
        # transmittance, k = 1 and k = 4
        t1 = _np(cam.transmittance(ts, spec, wavelengths=tl0))
        t4 = _np(cam.transmittance(ts, hero, wavelengths=tl))
        drv = host_drivers.transmittance()
        want1, want4 = np.zeros(len(s), F32), np.zeros(lam.shape, F32)
        want1[rows] = host_drivers.run_transmittance(drv, surf, disp, lam0[rows], o0, d0, coat, h2)
        want4[ti, tj] = host_drivers.run_transmittance(drv, surf, disp, lam[ti, tj], starts[ti, 0:3], starts[ti, 3:6], coat, h2)
        if not np.array_equal(bits(t1), bits(want1)) or not np.array_equal(bits(t4), bits(want4)):
            fail(tag + "transmittance against the host build: %d rows differ at k = 1, %d records at k = 4" % ((bits(t1) != bits(want1)).sum(), (bits(t4) != bits(want4)).sum()))
        if not (t1[rows] > 0).mean() > 0.5:
            fail(tag + "transmittance: only %.3f of the live rows let light through" % (t1[rows] > 0).mean())
        # ghosts
        some = pairs if len(pairs) <= MAX_PAIRS else pairs[np.unique(np.linspace(0, len(pairs) - 1, MAX_PAIRS).round().astype(int))]
        g = _words(cam.create_ghost_rays(ts, spec, some, wavelengths=tl0))
        want = bits(host_drivers.run_ghost_records(host_drivers.ghost(), L, disp, lam0, starts[:, 0:3], starts[:, 3:6], some, have=live, film=coat))
        if not np.array_equal(g, want):
            fail(tag + "ghosts against the host build: %d of %d records differ (first %s)" % ((g != want).any(2).sum(), g.shape[0] * g.shape[1], np.argwhere((g != want).any(2))[:4].tolist()))
        note["ghosts"] = dict(pairs=len(some), traced=int((want[..., 7] == 1).sum()), ended=int((want[..., 7] != 1).sum()))
        if note["ghosts"]["traced"] < 100:
            fail(tag + "only %d traced ghosts" % note["ghosts"]["traced"])
        # tangents
        d, c = (_np(t) for t in cam.ray_differentials(ts, spec, wavelengths=tl0, chromatic=True))
        out, ch, prim = host_drivers.run_differentials_spectral(host_drivers.differentials_spectral(), 2, surf, disp, hs, lam0[rows], o0, d0)
        if bits(d[~live]).any() or bits(c[~live]).any() or not (np.isfinite(d[rows]).all() and np.isfinite(c[rows]).all()):
            fail(tag + "differentials: a dead row that is not +0.0 or a live row that is not finite")
        if not np.array_equal(bits(c[rows]), bits(ch)):
            fail(tag + "the wavelength tangent differs from the host build on %d of %d rows" % ((bits(c[rows]) != bits(ch)).any(1).sum(), len(rows)))
        ref = dsc.reference(surf, disp, hs, lam0[rows], o0, d0)
        ro, rd = ref["end"]
        eo = np.linalg.norm(-ro - rec_s[rows, 0:3], axis=1) / np.linalg.norm(rec_s[rows, 0:3], axis=1)
        ed = np.linalg.norm(-rd - rec_s[rows, 3:6], axis=1) / np.linalg.norm(rec_s[rows, 3:6], axis=1)
        good = dsc.conditions(ref["cos"], eo, ed)[0]
        e = dref.rel_err(d[rows], out)[good]
        m = dsc.figures(d[rows], c[rows], ref, good)
        note["tangents"] = dict(m, host_med=float(np.median(e)), host_ok=float((e <= 1e-3).mean()))
        if not (np.median(e) <= 1e-5 and (e <= 1e-3).mean() >= 0.999):
            fail(tag + "screen tangents against the host build: median %.3g, within 1e-3: %.5f" % (np.median(e), (e <= 1e-3).mean()))
        if not (spectral_bounds_hold(m) if disp["cauchy_b"].any() else (m["s_med"] <= 1e-5 and m["s_ok"] >= 0.999)):
            fail(tag + "tangents against f64: %s" % (m,))
    # the d-line tangents (tests/test_differentials_gpu.py's bounds against the f64 finite differences from the recorded starts)
    dd = _np(cam.ray_differentials(ts, plain))
    e = dref.rel_err(dd[rows_d], dref.kolb_jacobian_fd(surf, hs, ref_d["starts"][rows_d, 0:3], ref_d["starts"][rows_d, 3:6]))
    note["d_line_tangents"] = dict(med=float(np.median(e)), ok=float((e <= 1e-3).mean()))
    if not (np.median(e) <= 1e-5 and (e <= 1e-3).mean() >= 0.999) or bits(dd[ref_d["weight"] == 0]).any():
        fail("d-line tangents against f64: median %.3g, within 1e-3: %.5f" % (np.median(e), (e <= 1e-3).mean()))
    D.state = state


def _dead_words(reason):
    rec = np.zeros(8, np.uint32)
    rec[7] = gref.flag_word(reason)
    return rec


def _dead(D, st, state, note):
    """THINLENS and NONE"""
    import torch
    fail, cam, oc, p = note["fail"].append, D.cam, D.oc, state.p
    info = cam.info()
    if len(cam.ghost_pairs()) != 0:
        fail("ghost_pairs() lists pairs for a lens without interfaces")
    thin = state.model == THINLENS
    pairs = np.array([(3, 1), (7, 0), (1, 3)], np.int32)
    if thin:
        k = D.__dict__.setdefault("thin_steps", 0)
        D.thin_steps = k + 1
        n = us.THIN_SIZES[k % len(us.THIN_SIZES)]
        s, lam, states = us.inputs(state.seed, n)
        ref_words, ref_counters, _ = hero_ref.hero_reference(D.oracle_lib, p, None, s, lam, states, details=True, oc=oc)
        ts, tl = _dev(s), _dev(lam)
        torch.cuda.synchronize()
        if k % 3:                                                            # two of the three sizes: two streams at once
            side = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = [cam.create_rays_hero(ts, tl, stream=q.cuda_stream)["rays"] for q in side]
            torch.cuda.synchronize()
            if not np.array_equal(_words(outs[0]), _words(outs[1])):
                fail("the hero call on two streams at once: the two results differ")
            hero = outs[0]
        else:
            hero = cam.create_rays_hero(ts, tl)["rays"]
        torch.cuda.synchronize()
        differ = ~hero_ref.same_words(_words(hero), ref_words)
        note.update(n=n, live=int((ref_words[:, 0, 6] != 0).sum()))
        if differ.any():
            fail("THINLENS hero call at n = %d: %d records differ from the reference (first %s)" % (n, differ.sum(), np.argwhere(differ)[:4].tolist()))
        # the dead answers of a lens without interfaces, on the rows of the call (hero_rows.flat's layout)
        s_r, lam_r = ts.repeat_interleave(us.K, 0).contiguous(), tl.contiguous().view(-1)
        st_r = _dev(np.repeat(states, us.K, 0))
        rays_r = hero.contiguous().view(-1, 8)
        liv = _np(rays_r)[:, 6] != 0
        d, c = (_np(t) for t in cam.ray_differentials(s_r, rays_r, wavelengths=lam_r, rng_states=st_r, chromatic=True))
        t = _np(cam.transmittance(s_r, rays_r, wavelengths=lam_r, rng_states=st_r))
        g = _words(cam.create_ghost_rays(s_r, rays_r, pairs, wavelengths=lam_r, rng_states=st_r))
        if bits(c).any() or bits(d[~liv]).any() or not (bits(d[liv]) != 0).any(1).all():
            fail("THINLENS differentials: a wavelength tangent, a dead row that is not +0.0 or a live row that is")
        if not np.array_equal(bits(t), bits(np.where(liv, F32(1.0), F32(0.0)))):
            fail("THINLENS transmittance is not 1.0 on the live rows and +0.0 elsewhere")
        if not (g == _dead_words(gref.MODEL)).all():
            fail("THINLENS ghosts are not ZOIC_GHOST_MODEL")
        # the d-line call on all N samples: the records the backward calls are given
        s_all, lam, states = us.inputs(state.seed)
        plain = _words(cam.create_rays(_dev(s_all))["rays"])
        ref = oc.create_rays(s_all, rng_states=states)
        if not hero_ref.same_words(plain, np.concatenate([bits(ref["planes"]).T, ref["flags"].astype(np.uint32)[:, None]], 1)).all():
            fail("THINLENS create_rays differs from the oracle")
        rec_d = plain[:, :7].copy().view(F32)
    else:
        s_all, lam, states = us.inputs(state.seed)
        ts, tl = _dev(s_all), _dev(lam)
        rec_d = np.zeros((len(s_all), 7), F32)
        rays = torch.zeros((len(s_all), 8), device="cuda")
        rays[:, 6] = 1.0
        for name, shape, call in (("create_rays", (len(s_all), 8), lambda out: cam.create_rays(ts, wavelengths=tl[:, 0].contiguous(), out=dict(rays=out))),
                                  ("create_rays_hero", (len(s_all), us.K, 8), lambda out: cam.create_rays_hero(ts, tl, out=dict(rays=out)))):
            out = torch.full(shape, float("nan"), device="cuda")
            got = us.status_of(lambda: call(out))
            torch.cuda.synchronize()
            if got != "INVALID_ARGUMENT" or not torch.isnan(out).all():
                fail("NONE: %s gave %s, wrote %d words" % (name, got, int((~torch.isnan(out)).sum())))
        d, c = (_np(t) for t in cam.ray_differentials(ts, rays, wavelengths=tl[:, 0].contiguous(), chromatic=True))
        t = _np(cam.transmittance(ts, rays, wavelengths=tl[:, 0].contiguous()))
        g = _words(cam.create_ghost_rays(ts, rays, pairs, wavelengths=tl[:, 0].contiguous()))
        if bits(d).any() or bits(c).any() or bits(t).any() or bits(_np(cam.ray_differentials(ts, rays))).any():
            fail("NONE: differentials or transmittance that are not +0.0")
        if not (g == _dead_words(gref.MODEL)).all():
            fail("NONE ghosts are not ZOIC_GHOST_MODEL")
    B = us.backward_inputs(info, state, rec_d, rec_d, lam[:, 0])
    B["live_d"] = B["live_s"] = rec_d[:, 6] != 0
    note["backward"] = _backward(fail, D, state, info, None, B, s_all)
    H = us.host_backward(cam, B)
    if state.model != THINLENS or not p["useDof"]:
        finite = np.isfinite(B["o"]).all(1) & np.isfinite(B["d"]).all(1) & (np.abs(B["d"]).sum(1) > 0)
        for call in ("trace_back", "trace_back_spectral", "jacobian", "jacobian_spectral"):
            if not (H[call][1][finite] == us.TRACE_BACK_MODEL << 8).all() or any(bits(np.ascontiguousarray(a)).any() for a in (H[call][0], *H[call][2:])):
                fail("%s: not ZOIC_TRACE_BACK_MODEL and zeros" % call)
    if state.model != THINLENS:
        for call in ("project", "project_spectral"):
            if not (H[call][1] == us.PROJECT_MODEL_NONE << 8).all() or bits(H[call][0]).any():
                fail("%s: not ZOIC_PROJECT_MODEL_NONE and zeros" % call)


def _failed(D, st, state, note):
    """every opt-in device call refuses and writes nothing"""
    import torch
    fail, cam = note["fail"].append, D.cam
    s, lam, _ = us.inputs(state.seed, 65)
    ts, tl = _dev(s), _dev(lam)
    tl0 = tl[:, 0].contiguous()
    n = len(s)
    rays = torch.zeros((n, 8), device="cuda")
    rays[:, 6] = 1.0
    hero = rays.view(n, 1, 8).expand(n, us.K, 8).contiguous()
    pts = torch.zeros((n, 3), device="cuda")
    pts[:, 2] = -100.0

    def fresh(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), device="cuda") if dtype == torch.float32 else torch.full(shape, -559038737, dtype=dtype, device="cuda")

    f32, i32 = fresh, lambda *shape: fresh(*shape, dtype=torch.int32)   # noqa: E731
    calls = {
        "create_rays(wavelengths=)": lambda o: cam.create_rays(ts, wavelengths=tl0, out=dict(rays=o[0])), "create_rays_hero": lambda o: cam.create_rays_hero(ts, tl, out=dict(rays=o[0])),
        "ray_differentials": lambda o: cam.ray_differentials(ts, rays, out=o[0]),
        "ray_differentials(wavelengths=)": lambda o: cam.ray_differentials(ts, rays, wavelengths=tl0, out=o[0]),
        "transmittance k = 1": lambda o: cam.transmittance(ts, rays, wavelengths=tl0, out=o[0]), "transmittance k = 4": lambda o: cam.transmittance(ts, hero, wavelengths=tl, out=o[0]),
        "create_ghost_rays": lambda o: cam.create_ghost_rays(ts, rays, np.array([(3, 1)]), wavelengths=tl0, out=o[0]),
        "project_points": lambda o: cam.project_points(pts, out=o[0], flags=o[1]), "project_points(wavelengths=)": lambda o: cam.project_points(pts, out=o[0], flags=o[1], wavelengths=tl0),
        "trace_back": lambda o: cam.trace_back(rays, out=o[0], flags=o[1]), "trace_back(wavelengths=)": lambda o: cam.trace_back(rays, out=o[0], flags=o[1], wavelengths=tl0),
        "trace_back_jacobian": lambda o: cam.trace_back_jacobian(rays, out=o[0], flags=o[1], jacobian=o[2]),
        "trace_back_jacobian(wavelengths=)": lambda o: cam.trace_back_jacobian(rays, wavelengths=tl0, out=o[0], flags=o[1], jacobian=o[2]),
    }
    outs = {"create_rays(wavelengths=)": [f32(n, 8)], "create_rays_hero": [f32(n, us.K, 8)], "ray_differentials": [f32(n, 12)], "ray_differentials(wavelengths=)": [f32(n, 12)],
            "transmittance k = 1": [f32(n)], "transmittance k = 4": [f32(n, us.K)], "create_ghost_rays": [f32(n, 1, 8)]}
    for name in calls:
        o = outs.get(name) or [f32(n, 2), i32(n)] + ([f32(n, 2, 6)] if "jacobian" in name else [])
        got = us.status_of(lambda: calls[name](o))
        torch.cuda.synchronize()
        written = sum(int((~torch.isnan(t)).sum()) if t.dtype == torch.float32 else int((t != -559038737).sum()) for t in o)
        if got != "NOT_UPDATED" or written:
            fail("%s on a camera that is not updated: %s, %d words written" % (name, got, written))
    if us.status_of(lambda: cam.create_rays(ts)) != "NOT_UPDATED":
        fail("create_rays on a camera that is not updated does not refuse")


@pytest.mark.parametrize("name,k", us.CASES, ids=us.IDS)
def test_step(gpu, oracle_lib, name, k):
    note = us.take(_DRIVERS, oracle_lib, name, k, 0, _raytraced, _dead, _failed)
    print(name, k, note["step"].name, us.figures_of(note))
    assert not note["fail"], "\n".join(note["fail"])

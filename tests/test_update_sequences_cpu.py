"""The opt-in calls after update sequences and setter changes, on tables-only cameras (no GPU): tests/update_sequences.py has the
scripts and their partners; tests/test_update_sequences_gpu.py runs the same scripts on the device.

One test per step of every sequence.  A step is taken when its test runs (the steps before it first), on ONE camera and ONE oracle
camera per sequence; what its checks find is collected and asserted empty, so a step that fails does not hide the ones after it.

A good RAYTRACED step:
  * info()'s lens arrays and exit-pupil LUT are the oracle's own, bit for bit (update_sequences.anchored); only then does info() feed
    the host drivers and the f64 restatements;
  * dispersion(), coatings() and ghost_pairs() are the expected tables, bit for bit, again after every group of setters applied with
    no update (`between`);
  * the conditions that keep the GPU module's step from hiding a failure, from the oracle alone: live records, companions that come
    through, retried heroes (per sequence), a coated step's transmittance differs from the bare one on more than half of its live
    rows, an override changes cauchy_b on two surfaces at least, the conditioning rule of the differentials tests leaves out at most
    5 % of the live rows, and the host build of csrc/differentials_spectral.hpp meets the bounds the kernel will be held to;
  * the six host single-item calls give the bits of a fresh twin and pass update_sequences.check_backward.
THINLENS and NONE steps: the twin, the host builds and the documented dead answers.  A failed step: the scripted status, every host
call ZOIC_ERR_NOT_UPDATED with its outputs untouched, and the next step's checks show that everything is back."""
import numpy as np
import pytest

from zoic_amd import RAYTRACED, THINLENS
from zoic_amd import _capi

import differentials_ref as dref
import differentials_spectral_corpus as dsc
import ghost_ref as gref
import host_drivers
import update_sequences as us
from device_cases import bits
from hero_ref import hero_reference
from hero_rows import spectral_bounds_hold
from transmittance_ref import housings

F32 = np.float32
_DRIVERS = {}


@pytest.fixture(scope="module", autouse=True)
def _cameras():
    yield
    for D in _DRIVERS.values():
        D.close()
    _DRIVERS.clear()


def _raytraced(D, st, state, note):
    fail, cam, oc, p = note["fail"].append, D.cam, D.oc, state.p
    for line in us.anchored(cam, oc, state):
        fail(line)
    bad, disp, film, pairs = us.tables_hold(cam, state)
    for line in bad:
        fail(line)
    info = cam.info()
    note["stop_limit"] = float(gref.lens(info)["housing2"][int(info["apertureElement"])])
    s, lam, states = us.inputs(state.seed)
    words, _, det = hero_reference(D.oracle_lib, p, disp, s, lam, states, details=True, oc=oc)
    w = words[:, :, 6].copy().view(F32)
    live = w[:, 0] != 0
    note.update(live=int(live.sum()), companions=int((w[:, 1:] != 0).sum()), retried=int((live & (((words[:, 0, 7] >> 1) & 31) > 0)).sum()))
    if note["live"] < us.MIN_LIVE or note["companions"] < us.MIN_COMPANIONS:
        fail("%d live records, %d companions that come through" % (note["live"], note["companions"]))
    rec_d = oc.create_rays(s, rng_states=states)["planes"].T
    rec_s = det["planes"].T
    B = us.backward_inputs(info, state, rec_d, rec_s, lam[:, 0])
    B["live_d"], B["live_s"] = rec_d[:, 6] != 0, live
    H = us.host_backward(cam, B)
    us.twin_holds(fail, D, state, cam, B, H)
    note["backward"] = us.check_backward(fail, cam, state, info, disp, B, H, s)
    us.reverse_ray_holds(fail, cam, state, B, H)
    # ---- the differentials' conditions and the host build's figures, from the recorded starts ----------------------------------------
    surf, hs = dref.surfaces(info), F32(F32(p["sensorWidth"]) * F32(0.5))
    rows = np.flatnonzero(live)
    o0, d0, lam0 = det["starts"][rows, 0:3], det["starts"][rows, 3:6], lam[rows, 0]
    ref = dsc.reference(surf, disp, hs, lam0, o0, d0)
    ro, rd = ref["end"]
    eo = np.linalg.norm(-ro - rec_s[rows, 0:3], axis=1) / np.linalg.norm(rec_s[rows, 0:3], axis=1)
    ed = np.linalg.norm(-rd - rec_s[rows, 3:6], axis=1) / np.linalg.norm(rec_s[rows, 3:6], axis=1)
    good, excluded, restated = dsc.conditions(ref["cos"], eo, ed)
    if excluded > 0.05 or not restated:
        fail("the conditioning rule leaves out %.4f of the live rows; the f64 restatement of the records holds: %s" % (excluded, restated))
    out, ch, prim = host_drivers.run_differentials_spectral(host_drivers.differentials_spectral(), 2, surf, disp, hs, lam0, o0, d0)
    m = dsc.figures(out, ch, ref, good)
    note["differentials"] = dict(m, excluded=excluded)
    if disp["cauchy_b"].any() and not spectral_bounds_hold(m):
        fail("the host build of differentials_spectral.hpp misses the bounds: %s" % (m,))
    if not disp["cauchy_b"].any() and not (m["s_med"] <= 1e-5 and m["s_ok"] >= 0.999):
        fail("the host build of differentials_spectral.hpp misses the screen tangents' bounds: %s" % (m,))
    # ---- overrides: at the update and between calls --------------------------------------------------------------------------------
    for group in [()] + list(st.between):
        us.apply(cam, state, group)
        bad, disp, film, pairs = us.tables_hold(cam, state)
        for line in bad:
            fail("after %s: %s" % ([g[0] for g in group], line))
        if group:
            H = us.host_backward(cam, B)
            us.twin_holds(fail, D, state, cam, B, H)
        if state.abbe is not None:
            plain = state.copy()
            plain.abbe = None
            changed = int((us.expected(plain)[0]["cauchy_b"] != disp["cauchy_b"]).sum())
            if changed < 2:
                fail("the override changes cauchy_b on %d surfaces" % changed)
        if state.coatings is not None:
            drv = host_drivers.transmittance()
            args = (drv, surf, disp, lam0, o0, d0)
            coated, bare = host_drivers.run_transmittance(*args, film, housings(info)), host_drivers.run_transmittance(*args, None, housings(info))
            share = float((bits(coated) != bits(bare)).mean())
            note["coated_share"] = share
            if share <= 0.5:
                fail("the coatings change the transmittance of %.3f of the live rows" % share)
    D.state = state


def _dead(D, st, state, note):
    """THINLENS and NONE"""
    fail, cam, oc, p = note["fail"].append, D.cam, D.oc, state.p
    info = cam.info()
    s, lam, states = us.inputs(state.seed)
    if len(cam.ghost_pairs()) != 0:
        fail("ghost_pairs() lists pairs for a lens without interfaces")
    if state.model == THINLENS:
        tl = oc.thinlens()
        if any(bits(F32(info[k])) != bits(F32(tl[k])) for k in ("tan_fov", "apertureRadius")):
            fail("tan_fov / apertureRadius differ from the oracle's")
        rec_d = oc.create_rays(s, rng_states=states)["planes"].T
    else:
        rec_d = np.zeros((len(s), 7), F32)
    B = us.backward_inputs(info, state, rec_d, rec_d, lam[:, 0])
    B["live_d"] = B["live_s"] = rec_d[:, 6] != 0
    H = us.host_backward(cam, B)
    us.twin_holds(fail, D, state, cam, B, H)
    note["backward"] = us.check_backward(fail, cam, state, info, None, B, H, s)
    us.reverse_ray_holds(fail, cam, state, B, H)
    dead_tb = state.model != THINLENS or not p["useDof"]
    if dead_tb:
        finite = np.isfinite(B["o"]).all(1) & np.isfinite(B["d"]).all(1) & (np.abs(B["d"]).sum(1) > 0)
        for call in ("trace_back", "trace_back_spectral", "jacobian", "jacobian_spectral"):
            if not (H[call][1][finite] == us.TRACE_BACK_MODEL << 8).all() or any(bits(np.ascontiguousarray(a)).any() for a in (H[call][0], *H[call][2:])):
                fail("%s: not ZOIC_TRACE_BACK_MODEL and zeros" % call)
    if state.model != THINLENS:
        for call in ("project", "project_spectral"):
            if not (H[call][1] == us.PROJECT_MODEL_NONE << 8).all() or bits(H[call][0]).any():
                fail("%s: not ZOIC_PROJECT_MODEL_NONE and zeros" % call)


@pytest.mark.parametrize("name,k", us.CASES, ids=us.IDS)
def test_step(oracle_lib, name, k):
    note = us.take(_DRIVERS, oracle_lib, name, k, -1, _raytraced, _dead)
    print(name, k, note["step"].name, us.figures_of(note))
    assert not note["fail"], "\n".join(note["fail"])


@pytest.mark.parametrize("name", list(us.SEQUENCES))
def test_a_step_of_every_sequence_has_retried_heroes(oracle_lib, name):
    steps = us.SEQUENCES[name][1]
    most = max(us.take(_DRIVERS, oracle_lib, name, k, -1, _raytraced, _dead).get("retried", 0) for k in range(len(steps)))
    assert most >= us.MIN_RETRIED, most


def test_the_f_stop_step_moves_the_stop_limit(oracle_lib):
    """the limit a stale ghost or backward table would still hold: up to f/5.6 the stop's own housing is the smaller one and an f-stop
    step would change nothing"""
    steps = [st.name for st in us.SEQUENCES["parameters"][1]]
    k = steps.index("fstop")
    before, after = (us.take(_DRIVERS, oracle_lib, "parameters", j, -1, _raytraced, _dead)["stop_limit"] for j in (k - 1, k))
    assert after < 0.9 * before, (before, after)


def test_the_scripts_hold_every_transition():
    """every item of the list the scripts were written from appears in one of them"""
    steps = [st for _, seq in us.SEQUENCES.values() for st in seq]
    changed = [set(st.params) for st in steps]
    for alone in ("fStop", "focalDistance", "focalLength", "sensorWidth", "kolbSamplingLUT", "exposureControl"):
        assert {alone} in changed, alone
    assert any({"useDof", "opticalVignettingDistance", "opticalVignettingRadius"} <= c for c in changed)
    assert any(not st.params and not st.setters and not st.between for st in steps[1:])                     # an update that changes nothing
    setters = [what for st in steps for what, _ in st.setters] + [what for st in steps for g in st.between for what, _ in g]
    for what in ("abbe", "coatings", "precision", "seed", "reverse", "image", "lens_text"):
        assert what in setters, what
    assert sum(1 for st in steps for what, _ in st.setters if what == "image") >= 2                         # on, replaced
    assert any(v is None for st in steps for g in st.between for _, v in g)                                # count = 0 between two passes
    assert {st.status for st in steps} >= {None, "INVALID_ARGUMENT", "LENS_PARSE", "LENS_PATH"}
    models = [st.params.get("lensModel") for st in us.SEQUENCES["models"][1]]
    assert [m for m in models if m is not None] == [THINLENS, _capi.LENS_NONE, RAYTRACED, THINLENS]
    assert all(st.reason for st in steps) and 6 <= len(us.SEQUENCES) <= 8 and all(6 <= len(seq) <= 9 for _, seq in us.SEQUENCES.values())

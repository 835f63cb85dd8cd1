"""Scripted update histories of ONE camera, for tests/test_update_sequences_cpu.py and tests/test_update_sequences_gpu.py: a helper,
not a test.

Every opt-in call (spectral and hero rays, differentials, transmittance, ghosts, projection, trace-back and its Jacobian) answers from
state that zoic_camera_update derived (the kolb / thin tables, cam->reverse, cam->traceBack, cam->ghost and its device copy), from
state derived at the call (the dispersion and film tables of the overrides, the precision mode, the seed) or from state kept across
calls (the hero staging buffer).  The single-update modules create a camera, update it once and use it.  Here a camera lives through
SEQUENCES: lists of steps, each (setter calls, parameter changes, expected status, setter calls between two calls) with its reason.

The partners of a step:
  * an OracleCamera driven through the same updates (Driver.oc): the exit-pupil LUT is sampled from a generator that runs on, so only
    a camera with the same history has the same start rays.  Lock-step needs care where the two differ by design:
      - a step scripted to fail in the PARSE or at the PATH leaves the oracle alone (`oracle=False`): the library draws nothing there
        and rebuilds at the next update, so the recovering step changes the lens and the oracle rebuilds once, as the library does;
      - a step that fails on an override's COUNT fails after the lens was rebuilt (the library has drawn its LUT), and the library
        rebuilds again at the next update, whatever it changes: the oracle takes that step's update (it knows no overrides) and the
        recovering step changes a lens parameter, two rebuilds on both sides;
      - the oracle looks at lensDataPath, not at the text (zoic.cpp:595-611), so a step that gives a text changes the path too.
  * the expected tables (expected()): the dispersion table from the step's prescription text, the V-number override and
    spectral_ref.cauchy_b; the film table from the coatings override; the pairs from ghost_ref.expected_pairs;
  * a fresh twin (Driver.twin()): a tables-only camera brought straight to the step's state, for what does not depend on the LUT's
    history (projection, trace-back, the Jacobian, their spectral forms, the three getters)."""
from collections import namedtuple

import numpy as np

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, RAYTRACED, THINLENS, ZoicCamera, lens_path
from zoic_amd._capi import LENS_NONE
from zoic_amd.camera import ZoicError
from zoic_amd.workloads import hexagon_bokeh, ray_rng_states

import backward_spectral_ref as bs
import device_cases as dc
import ghost_ref as gref
import host_drivers
import traceback_cases as tc
import traceback_jacobian_ref as jr
from fuzz_cameras import CUSTOM_LENS_5, bokeh_image, rows_of
from reverse_ref import kolb_point_set, thin_point_set
from spectral_ref import cauchy_b
from traceback_ref import TraceBack

F32 = np.float32
N = 2048 + 65                      # 33 waves and one lane more: more than one block, a partial last wave
K = 4
PALETTE = np.array([400.0, 486.1327, 587.5618, 656.2725, 700.0], F32)
THIN_SIZES = (65, N, 63)           # the hero calls of the THINLENS steps, in step order: the staging buffer grows, then is reused
MIN_LIVE, MIN_COMPANIONS, MIN_RETRIED = 256, 32, 32

TESSAR, GAUSS, PETZVAL, MORI, TRIPLET = ("tessar_f2.8.dat", "double_gauss_f2.0.dat", "petzval_f1.25.dat", "mori_f2.8.dat", "triplet_f2.5.dat")
# rows of the prescriptions (the length an override must have): TESSAR 8, GAUSS / PETZVAL / MORI 11, TRIPLET 7, the text "four" 5
TEXTS = {"four": CUSTOM_LENS_5, "garbage": "40.0\t2.0\t1.6\t20.0\n-200.0\tthree\t0.0\t20.0\n0\t5.0\t0\t12.0\n"}
IMAGES = {"hexagon": hexagon_bokeh, "spots": lambda: bokeh_image(37, 53, "spots", 11)}
MISSING = "/nowhere/zoic/no_such_lens.dat"

BASE = dict(lensModel=RAYTRACED, lensDataPath=lens_path(TESSAR), focalLength=5.0, fStop=2.8, focalDistance=100.0, sensorWidth=3.6,
            sensorHeight=2.4, kolbSamplingLUT=True, useImage=False, bokehPath="", useDof=True, exposureControl=0.0,
            opticalVignettingDistance=0.0, opticalVignettingRadius=1.0)


def V(count, salt=0):
    """V-numbers in file order for a lens of `count` rows: 24 ... 68, no two alike, another order per salt"""
    return np.roll(np.linspace(24.0, 68.0, count), salt).astype(F32)


def films(count, salt=0):
    """coatings in file order: every interface coated (index 1.38 or 1.46), quarter-wave at 480 ... 620 nm"""
    return (np.where((np.arange(count) + salt) % 3 == 0, 1.46, 1.38).astype(F32), np.roll(np.linspace(480.0, 620.0, count), salt).astype(F32))


Step = namedtuple("Step", "name reason setters params status oracle between")


def step(name, reason, setters=(), params=None, status=None, oracle=True, between=()):
    """setters: (what, value) pairs applied before the update -- abbe (V-numbers or None), coatings ((index, lambda0) or None), precision,
    seed, reverse, image (a key of IMAGES), lens_text (a key of TEXTS or None); params: parameters that change; status: the status name
    the update must give (None: ZOIC_OK); oracle: the oracle camera takes the update; between: lists of setters, each applied after
    the forward calls with no update, the passes run again after each"""
    return Step(name, reason, tuple(setters), dict(params or {}), status, oracle, tuple(tuple(b) for b in between))


def _lens(name):
    return dict(lensDataPath=lens_path(name))


SEQUENCES = {
    "parameters": (TESSAR, [
        step("first", "the state every single-update module stops at"),
        step("exposure", "rebuilds no lens: the backward and ghost tables must still be there, kolb.exposure must follow", params=dict(exposureControl=1.5)),
        step("dof-vignetting", "rebuilds no lens; RAYTRACED reads neither", params=dict(useDof=False, opticalVignettingDistance=3.0, opticalVignettingRadius=0.8)),
        step("fstop", "alone: f/8 moves the stop limit of every backward table and of the ghost table (up to f/5.6 the stop's housing is the limit)", params=dict(fStop=8.0)),
        step("focus", "alone: moves originShift", params=dict(focalDistance=55.0)),
        step("focal", "alone: rescales the lens", params=dict(focalLength=7.0)),
        step("sensor", "alone: normalises Ps", params=dict(sensorWidth=2.8)),
        step("lut-off", "alone: the LUT switch owns flag bit 2; every hero is retried from the disk", params=dict(kolbSamplingLUT=False)),
        step("same", "an update that changes nothing"),
    ]),
    "image": (GAUSS, [
        step("first", "four-column prescription: no V-numbers, no colour"),
        step("image-on", "a bokeh image rebuilds the lens (zoic.cpp:595-611) and changes every start", [("image", "hexagon")], dict(useImage=True, bokehPath="mem:hexagon")),
        step("image-replaced", "new pixels under a new path", [("image", "spots")], dict(bokehPath="mem:spots")),
        step("exposure", "rebuilds neither lens nor image", params=dict(exposureControl=-1.0)),
        step("abbe", "an override on the four-column lens, set before an update that rebuilds nothing", [("abbe", V(11))]),
        step("image-off", "back to the disk sampler", params=dict(useImage=False)),
        step("lut-off", "retried heroes", params=dict(kolbSamplingLUT=False)),
    ]),
    "overrides": (PETZVAL, [
        step("first", "both overrides set before the first update", [("abbe", V(11)), ("coatings", films(11))]),
        step("equal-count", "another prescription of 11 rows: both overrides apply, reversed, to the NEW glasses", params=_lens(MORI)),
        step("other-count", "8 rows under overrides of 11: the update fails after the lens was rebuilt", params=_lens(TESSAR), status="INVALID_ARGUMENT"),
        step("cleared", "recovered by clearing both overrides", [("abbe", None), ("coatings", None)], dict(fStop=3.2)),
        step("stale-override", "V-numbers of 8 accepted for the lens of 8, then a lens of 11", [("abbe", V(8, 3))], _lens(GAUSS), status="INVALID_ARGUMENT"),
        step("new-length", "recovered by passing one of the new length to the camera that is not updated", [("abbe", V(11, 5))], dict(focalDistance=80.0)),
        step("coated-lut-off", "coatings before an update that rebuilds for another reason", [("coatings", films(11, 1))], dict(kolbSamplingLUT=False)),
    ]),
    "between-calls": (TESSAR, [
        step("first", "bare, the prescription's own V-numbers"),
        step("same", "overrides set and cleared between a forward call and its passes and between two passes: read at the call",
             between=[[("abbe", V(8))], [("coatings", films(8))], [("abbe", None)], [("coatings", None)]]),
        step("fast-seed", "precision and seed are read at the call", [("precision", PRECISION_FAST), ("seed", 7)], dict(fStop=3.5)),
        step("strict-seed", "and back, before an update that rebuilds nothing", [("precision", PRECISION_STRICT), ("seed", 12345)], dict(exposureControl=0.5)),
        step("reverse-on", "camera_reverse_ray answers with the projection of the CURRENT tables", [("reverse", True)], dict(kolbSamplingLUT=False)),
        step("reverse-off", "and is False again", [("reverse", False)], dict(sensorWidth=3.0)),
        step("text", "a four-column text, then V-numbers for it with no update between", [("lens_text", "four")], dict(lensDataPath="text:four", kolbSamplingLUT=True),
             between=[[("abbe", V(5))], [("coatings", films(5, 2))]]),
    ]),
    "models": (TESSAR, [
        step("first", "RAYTRACED, coated and overridden: what the other models must not answer from", [("abbe", V(8, 1)), ("coatings", films(8))]),
        step("thin", "THINLENS: the hero staging buffer's first use, k = 4 at n = 65", params=dict(lensModel=THINLENS)),
        step("thin-vignetting", "rebuilds nothing: the THINLENS trace-back reads the vignetting pair; n = 2113, the buffer grows",
             params=dict(opticalVignettingDistance=5.0, opticalVignettingRadius=0.9)),
        step("thin-pinhole", "useDof off: ZOIC_TRACE_BACK_MODEL; n = 63 in the grown buffer", params=dict(useDof=False)),
        step("none", "NONE: every dead answer", params=dict(lensModel=LENS_NONE)),
        step("raytraced", "back: the lens, its tables and the overrides of step 0 are all there again", params=dict(lensModel=RAYTRACED, useDof=True, kolbSamplingLUT=False)),
        step("thin-again", "the staging buffer after a RAYTRACED step", params=dict(lensModel=THINLENS)),
    ]),
    "failures": (GAUSS, [
        step("first", "a good camera"),
        step("parse", "a text that does not parse", [("lens_text", "garbage")], status="LENS_PARSE", oracle=False),
        step("recovered", "the text taken back, another prescription", [("lens_text", None)], _lens(TRIPLET)),
        step("path", "a path that is not there", params=dict(lensDataPath=MISSING), status="LENS_PATH", oracle=False),
        step("recovered-again", "a good path", [("coatings", films(11))], _lens(PETZVAL)),
        step("exposure", "rebuilds nothing after a recovery", params=dict(exposureControl=-0.5)),
        step("lut-off", "retried heroes", params=dict(kolbSamplingLUT=False)),
    ]),
}
CASES = [(name, k) for name, (_, steps) in SEQUENCES.items() for k in range(len(steps))]
IDS = ["%s-%d-%s" % (name, k, SEQUENCES[name][1][k].name) for name, k in CASES]


def inputs(seed, n=N):
    """(samples (n,4), wavelengths (n,K): the palette, the hero's in column 0, rng states (n,4) of `seed`)"""
    s = dc.samples(N)[:n]
    i = np.arange(n)[:, None]
    lam = PALETTE[(i + 2 * np.arange(K)[None, :]) % len(PALETTE)]
    return s, np.ascontiguousarray(lam, F32), ray_rng_states(n, seed=seed)


class State:
    """what a step leaves behind: the parameters, the overrides (file order), the prescription's rows, the switches"""

    def __init__(self, lens):
        self.p = dict(BASE, **_lens(lens))
        self.abbe = self.coatings = self.text = self.image = None
        self.precision, self.seed, self.reverse = PRECISION_STRICT, 1, False
        self.updated = False

    def copy(self):
        c = State.__new__(State)
        c.__dict__.update(self.__dict__)
        c.p = dict(self.p)
        return c

    @property
    def model(self):
        return self.p["lensModel"]

    @property
    def raytraced(self):
        return self.updated and self.model == RAYTRACED

    def rows(self):
        """the prescription's rows, file order"""
        return rows_of(TEXTS[self.text]) if self.text is not None else rows_of(self.p["lensDataPath"])


def expected(state):
    """(dispersion dict of ior_d, abbe, cauchy_b; film (index, lambda0); pairs) of a RAYTRACED state, trace order, from the prescription
    text and the overrides alone"""
    rows = state.rows()[::-1]
    ior = np.array([r[2] if r[2] != 0.0 else 1.0 for r in rows], F32)
    abbe = np.array([r[3] if len(r) == 5 else 0.0 for r in rows], F32)
    if state.abbe is not None:
        assert len(state.abbe) == len(rows)
        abbe = np.ascontiguousarray(state.abbe[::-1], F32)
    disp = dict(ior_d=ior, abbe=abbe, cauchy_b=cauchy_b(ior, abbe))
    film = (np.zeros(len(rows), F32), np.zeros(len(rows), F32))
    if state.coatings is not None:
        film = (np.ascontiguousarray(state.coatings[0][::-1], F32), np.ascontiguousarray(state.coatings[1][::-1], F32))
    return disp, film, gref.expected_pairs(disp)


def status_of(call):
    """the status name of a library call without its prefix, None for ZOIC_OK"""
    try:
        call()
    except ZoicError as e:
        return e.status_name.replace("ZOIC_ERR_", "")
    return None


def apply(cam, state, setters, oc=None):
    """apply setters to the camera (and the oracle, where it has the setter) and note them in the state"""
    for what, value in setters:
        if what == "abbe":
            cam.set_abbe_numbers(value)
            state.abbe = value
        elif what == "coatings":
            cam.set_coatings(*(value if value is not None else (None, None)))
            state.coatings = value
        elif what == "precision":
            cam.set_precision(value)
            state.precision = value
        elif what == "seed":
            cam.set_seed(value)
            state.seed = value
        elif what == "reverse":
            cam.set_reverse_projection(value)
            state.reverse = value
        elif what == "image":
            px = IMAGES[value]()
            cam.set_bokeh_image(px)
            if oc is not None:
                oc.set_bokeh_image(px)
            state.image = value
        elif what == "lens_text":
            cam.set_lens_text(None if value is None else TEXTS[value])
            if oc is not None and value is not None and TEXTS[value] is not TEXTS["garbage"]:
                oc.set_lens_text(TEXTS[value])
            state.text = value
        else:
            raise KeyError(what)


class Driver:
    """one camera and one oracle camera walked through a sequence; step k is taken once, in order"""

    def __init__(self, oracle_lib, name, device):
        self.oracle_lib, self.name, self.device = oracle_lib, name, device
        lens, self.steps = SEQUENCES[name]
        self.cam, self.oc = ZoicCamera(device=device), oracle_lib.OracleCamera()
        self.state = State(lens)
        self.done = -1
        self.broken = None          # the step whose checks raised something unexpected: the camera's later steps are void
        self.seen = {}              # step index -> what the module's checks noted (their failures among it)

    def update(self, k):
        """take step k's setters and update: (step, state after, status name of the library's update)"""
        assert k == self.done + 1, "steps are taken in order"
        st = self.steps[k]
        apply(self.cam, self.state, st.setters, self.oc)
        self.state.p.update(st.params)
        got = status_of(lambda: self.cam.update(**self.state.p))
        if st.oracle:
            self.oc.update(**self.state.p)
        self.state.updated = got is None
        self.done = k
        return st, self.state.copy(), got

    def twin(self, state):
        """a fresh tables-only camera brought straight to `state`"""
        cam = ZoicCamera(device=-1)
        if state.text is not None:
            cam.set_lens_text(TEXTS[state.text])
        if state.p.get("useImage"):
            cam.set_bokeh_image(IMAGES[state.image]())
        if state.abbe is not None:
            cam.set_abbe_numbers(state.abbe)
        if state.coatings is not None:
            cam.set_coatings(*state.coatings)
        cam.set_reverse_projection(state.reverse)
        cam.update(**state.p)
        return cam

    def close(self):
        self.cam.close()
        self.oc.close()


def anchored(cam, oc, state):
    """the failures of `cam.info()` against the oracle's own tables, bit for bit: the lens arrays (zo_lenses and the derived scalars)
    and, with the LUT on, its keys and boxes.  From there on info() may feed the host drivers and the f64 restatements."""
    bad = []
    info, lt = cam.info(), oc.lens_table()
    if info["lensCount"] != lt["lensCount"] or info["apertureElement"] != lt["apertureElement"]:
        return ["lens count / stop: %s against the oracle's %s" % ((info["lensCount"], info["apertureElement"]), (lt["lensCount"], lt["apertureElement"]))]
    if not np.array_equal(dc.bits_f32(info["elements"]), dc.bits_f32(lt["elements"])):
        bad.append("lens elements differ from zo_lenses")
    for key in ("userApertureRadius", "originShift", "apertureDistance", "focalLengthRatio"):
        if dc.bits_f32(info[key]) != dc.bits_f32(lt[key]):
            bad.append("%s %r against the oracle's %r" % (key, info[key], lt[key]))
    keys, boxes = oc.lut()
    if state.p["kolbSamplingLUT"]:
        if len(keys) == 0 or not np.array_equal(dc.bits_f32(info["lutBoxes"]), dc.bits_f32(boxes)) or not np.array_equal(dc.bits_f32(info["lutKeys"]), dc.bits_f32(keys)):
            bad.append("exit-pupil LUT differs from the oracle's")
    return bad


def tables_hold(cam, state):
    """the failures of dispersion(), coatings() and ghost_pairs() against expected(state), bit for bit; and the expected tables"""
    disp, film, pairs = expected(state)
    bad = []
    got = cam.dispersion()
    for key in ("ior_d", "abbe", "cauchy_b"):
        if got[key].shape != disp[key].shape or not np.array_equal(dc.bits_f32(got[key]), dc.bits_f32(disp[key])):
            bad.append("dispersion()[%s] %s, expected %s" % (key, got[key], disp[key]))
    c = cam.coatings()
    if c["index"].shape != film[0].shape or not np.array_equal(dc.bits_f32(c["index"]), dc.bits_f32(film[0])) or not np.array_equal(dc.bits_f32(c["lambda0_nm"]), dc.bits_f32(film[1])):
        bad.append("coatings() %s, expected %s" % (c, film))
    gp = cam.ghost_pairs()
    if gp.shape != pairs.shape or not np.array_equal(gp, pairs):
        bad.append("ghost_pairs(): %d pairs, expected %d" % (len(gp), len(pairs)))
    return bad, disp, film, pairs


# ---- the backward calls ----------------------------------------------------------------------------------------------------------
EDGE_CAP = 0.02                    # tests/test_traceback_cpu.py, tests/test_backward_spectral_cpu.py
MAX_POINTS = 512


def backward_inputs(info, state, rec_d, rec_s, lam0):
    """What a step's backward calls are given: rays (o, d, lam) -- the step's own forward records, d-line (rec_d) and at the palette
    (rec_s, wavelengths lam0), every one whatever its weight, 256 of traceback_cases.random_lines and the non-finite rays, the last two
    at the palette in turn -- and points (pts, plam, screen samples or None): a stride of reverse_ref's point set of the camera"""
    n = len(rec_d)
    ol, dl = tc.random_lines(info, 256)
    on, dn = tc.non_finite_rays()
    o = np.concatenate([rec_d[:, 0:3], rec_s[:, 0:3], ol, on]).astype(F32)
    d = np.concatenate([rec_d[:, 3:6], rec_s[:, 3:6], dl, dn]).astype(F32)
    extra = PALETTE[np.arange(len(ol) + len(on)) % len(PALETTE)]
    lam = np.concatenate([np.full(n, PALETTE[2], F32), lam0, extra]).astype(F32)
    smp = None
    if state.model == RAYTRACED:
        pts, smp, _ = kolb_point_set(info, state.p["sensorWidth"], state.p["focalDistance"])
    elif state.model == THINLENS:
        pts, smp, _ = thin_point_set(float(info["tan_fov"]), state.p["focalDistance"])
    else:
        pts = np.random.RandomState(3).uniform(-50, 50, (64, 3)).astype(F32)
    if len(pts) < 24:               # (the Mori lens at this focal length: no image circle of unclipped chief rays to take points from)
        live = np.flatnonzero(rec_d[:, 6] != 0)[:MAX_POINTS]
        pts, smp = (rec_d[live, 0:3] + F32(150.0) * rec_d[live, 3:6]).astype(F32), None
    pick = np.unique(np.linspace(0, len(pts) - 1, min(len(pts), MAX_POINTS)).astype(int))
    pts = np.ascontiguousarray(pts[pick], F32)
    smp = None if smp is None else np.asarray(smp, np.float64)[pick]
    return dict(o=o, d=d, lam=lam, n=n, pts=pts, plam=PALETTE[np.arange(len(pts)) % len(PALETTE)], smp=smp)


CALLS = ("trace_back", "trace_back_spectral", "project", "project_spectral", "jacobian", "jacobian_spectral")


def host_backward(cam, B):
    """the six host single-item calls on backward_inputs B: name -> tuple of arrays"""
    return {"trace_back": tc.lib_trace(cam, B["o"], B["d"]), "trace_back_spectral": tc.lib_trace(cam, B["o"], B["d"], B["lam"]),
            "project": tc.lib_project(cam, B["pts"]), "project_spectral": tc.lib_project(cam, B["pts"], B["plam"]),
            "jacobian": jr.host_jacobian(cam, B["o"], B["d"]), "jacobian_spectral": jr.host_jacobian(cam, B["o"], B["d"], B["lam"])}


def differing(a, b):
    """the calls of two host_backward-shaped results that are not the same bits, with the number of items that differ"""
    out = []
    for call in CALLS:
        rows = np.zeros(len(a[call][0]), bool)
        for x, y in zip(a[call], b[call]):
            x, y = dc.bits(np.ascontiguousarray(x)).reshape(len(rows), -1), dc.bits(np.ascontiguousarray(y)).reshape(len(rows), -1)
            rows |= (x != y).any(1)
        if rows.any():
            out.append("%s: %d of %d items differ (first %s)" % (call, rows.sum(), len(rows), np.flatnonzero(rows)[:4].tolist()))
    return out


def check_backward(fail, cam, state, info, disp, B, H, samples):
    """The host single-item results H = host_backward(cam, B) of an updated camera against
      * the host builds of csrc/traceback.hpp and csrc/reverse.hpp filled from the ANCHORED info() and the step's parameters, bit for bit
        (the d-line calls): a backward table that was not refilled, or refilled from something else, differs here;
      * the identities: the Jacobian calls' (Ps, flags) are the trace-back calls', the Jacobian is +0.0 where bit 0 is clear, the calls
        at 587.5618 nm are the d-line calls;
      * RAYTRACED / THINLENS: the f64 restatements built from the anchored info() with the bounds of the single-update modules --
        tests/test_traceback_cpu.py (|lib - f64| <= 4 E_ref max and p99, round trip of the records <= 5 E_ref max, E_ref the f64
        trace-back of the ORACLE's records against their samples: reference against reference; decisions equal off the edge set, which
        is at most EDGE_CAP), tests/test_backward_spectral_cpu.py (at the palette at most 2 x the d-line figure) and
        tests/test_reverse_cpu.py (projection of the chief-ray point set: max 1e-5, p99 2e-6, at the palette 2 x the d-line max)."""
    p, n = state.p, B["n"]
    scr, fl = host_drivers.drive_traceback(host_drivers.traceback(), cam, p, B["o"], B["d"])
    if not (np.array_equal(dc.bits(scr), dc.bits(H["trace_back"][0])) and np.array_equal(fl, H["trace_back"][1])):
        fail("trace_back_ray is not the host build of traceback.hpp from info() and the parameters: %d rays" % (
            (dc.bits(scr) != dc.bits(H["trace_back"][0])).any(1) | (fl != H["trace_back"][1])).sum())
    scr, fl = host_drivers.drive_reverse(host_drivers.reverse(), cam, p, B["pts"])
    if not (np.array_equal(dc.bits(scr), dc.bits(H["project"][0])) and np.array_equal(fl, H["project"][1])):
        fail("project_point is not the host build of reverse.hpp from info() and the parameters")
    for a, b in (("jacobian", "trace_back"), ("jacobian_spectral", "trace_back_spectral")):
        if not (np.array_equal(dc.bits(H[a][0]), dc.bits(H[b][0])) and np.array_equal(H[a][1], H[b][1])):
            fail("%s: (Ps, flags) are not %s's" % (a, b))
        if dc.bits(H[a][2][(H[a][1] & 1) == 0]).any():
            fail("%s: a Jacobian that is not +0.0 on a ray that is not traced back" % a)
    dl = B["lam"] == PALETTE[2]
    for a, b in (("trace_back_spectral", "trace_back"), ("jacobian_spectral", "jacobian")):
        for x, y in zip(H[a], H[b]):
            if not np.array_equal(dc.bits(np.ascontiguousarray(x[dl])), dc.bits(np.ascontiguousarray(y[dl]))):
                fail("%s at 587.5618 nm is not %s" % (a, b))
    if state.model not in (RAYTRACED, THINLENS) or (state.model == THINLENS and not p["useDof"]):
        return None
    # ---- f64, d-line: the records' round trip -------------------------------------------------------------------------------------
    T = bs.SpectralTraceBack(info, p, disp) if state.model == RAYTRACED else TraceBack(info, p)
    live = np.flatnonzero(np.isfinite(B["o"][:n]).all(1) & (np.abs(B["d"][:n]).sum(1) > 0) & B["live_d"])
    o, d, smp = B["o"][live], B["d"][live], samples[live, :2].astype(np.float64)
    ref = T.trace(o, d)
    edge = T.edge(ref)
    good = ~edge & ref["traced"]
    e_ref = np.abs(ref["ps"] - smp).max(1)
    e_max, e_p99 = float(e_ref[good].max()), float(np.percentile(e_ref[good], 99))
    ps, flg = H["trace_back"][0][live], H["trace_back"][1][live]
    ok = (flg & 1) == 1
    if edge.mean() > EDGE_CAP or len(live) < MIN_LIVE:
        fail("d-line records: %d live, edge share %.4f" % (len(live), edge.mean()))
    if state.model == RAYTRACED and ((~edge & ~ref["traced"]).any() or (~edge & ~ok).any()):
        fail("d-line records off the edge refused: f64 %d, library %d" % ((~edge & ~ref["traced"]).sum(), (~edge & ~ok).sum()))
    if not np.array_equal(ok[~edge], ref["traced"][~edge]):
        fail("d-line decisions differ from the f64 trace on %d non-edge records" % (ok[~edge] != ref["traced"][~edge]).sum())
    both = good & ok
    err = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
    rt = np.abs(ps.astype(np.float64) - smp).max(1)[both]
    out = dict(e_max=e_max, e_p99=e_p99, err_max=float(err.max()), err_p99=float(np.percentile(err, 99)), rt_max=float(rt.max()), live=live, edge=edge, both=both)
    if both.sum() < 0.97 * len(live) or err.max() > 4.0 * e_max or np.percentile(err, 99) > 4.0 * e_p99 or rt.max() > 5.0 * e_max:
        fail("d-line trace-back against f64: %d of %d compared, |lib - f64| max %.3g p99 %.3g, round trip max %.3g; E_ref max %.3g p99 %.3g" % (
            both.sum(), len(live), err.max(), np.percentile(err, 99), rt.max(), e_max, e_p99))
    if dc.bits(H["trace_back"][0][(H["trace_back"][1] & 1) == 0]).any():
        fail("a refused ray with Ps that is not (+0.0, +0.0)")
    if state.model != RAYTRACED:
        return out
    # ---- f64 at the palette: the spectral records' round trip --------------------------------------------------------------------
    lv = np.flatnonzero(B["live_s"])
    o, d, lam = B["o"][n + lv], B["d"][n + lv], B["lam"][n + lv]
    ref = T.trace_at(o, d, lam)
    edge = T.edge(ref)
    ps, flg = H["trace_back_spectral"][0][n + lv], H["trace_back_spectral"][1][n + lv]
    ok = (flg & 1) == 1
    both = ~edge & ok & ref["traced"]
    if edge.mean() > EDGE_CAP or not np.array_equal(ok[~edge], ref["traced"][~edge]) or both.sum() < 0.97 * len(lv):
        fail("palette records: edge share %.4f, %d decisions differ off the edge, %d of %d compared" % (
            edge.mean(), (ok[~edge] != ref["traced"][~edge]).sum(), both.sum(), len(lv)))
    err_s = np.abs(ps.astype(np.float64) - ref["ps"]).max(1)[both]
    rt_s = np.abs(ps.astype(np.float64) - samples[lv, :2].astype(np.float64)).max(1)[both]
    out.update(err_s_max=float(err_s.max()), rt_s_max=float(rt_s.max()))
    if err_s.max() > 2.0 * out["err_max"] or rt_s.max() > 2.0 * 5.0 * e_max:
        fail("palette trace-back against f64: max %.3g (d-line %.3g), round trip %.3g (E_ref max %.3g)" % (err_s.max(), out["err_max"], rt_s.max(), e_max))
    # ---- projection ------------------------------------------------------------------------------------------------------------------
    scr, flg = H["project"]
    proj = (flg & 1) == 1
    if B["smp"] is not None:
        perr = np.abs(scr[proj].astype(np.float64) - B["smp"][proj]).max(1)
        out.update(p_cover=float(proj.mean()), p_max=float(perr.max()), p_p99=float(np.percentile(perr, 99)))
        if proj.mean() < 1.0 or perr.max() > 1e-5 or np.percentile(perr, 99) > 2e-6 or (flg[proj] & 2).any():
            fail("projection of the chief-ray points: cover %.4f, max %.3g, p99 %.3g" % (proj.mean(), perr.max(), np.percentile(perr, 99)))
    if B["smp"] is None:            # points off the forward rays: inside no single-update module's point set, held to the bits alone
        return out
    pick = np.arange(0, len(B["pts"]), max(1, len(B["pts"]) // 64))          # the f64 chief-ray search is a bisection per point
    worst = {}
    for key, lam in (("project", np.full(len(pick), bs.LAMBDA_D)), ("project_spectral", B["plam"][pick].astype(np.float64))):
        ref_ps, ok_ref = np.zeros((len(pick), 2)), np.zeros(len(pick), bool)
        for w in np.unique(lam):
            rows = np.flatnonzero(lam == w)
            ref_ps[rows], ok_ref[rows] = bs.project_at(info, p["sensorWidth"], disp, B["pts"][pick[rows]], float(w))
        okl = (H[key][1][pick] & 1) == 1
        if ok_ref.mean() < 0.99 or not okl[ok_ref].all():
            fail("%s: the f64 chief ray projects %.3f of the points, the library refuses %d of them" % (key, ok_ref.mean(), (~okl[ok_ref]).sum()))
        worst[key] = float(np.abs(H[key][0][pick].astype(np.float64) - ref_ps).max(1)[okl & ok_ref].max())
    out.update(pf64=worst["project"], pf64_s=worst["project_spectral"])
    if worst["project_spectral"] > 2.0 * worst["project"]:
        fail("projection at the palette against f64: max %.3g, d-line %.3g" % (worst["project_spectral"], worst["project"]))
    return out


# ---- a camera that is not updated ------------------------------------------------------------------------------------------------
NOT_UPDATED = 9
TRACE_BACK_MODEL, PROJECT_MODEL_NONE, GHOST_MODEL = 6, 4, 9     # include/zoic_amd.h: the dead answers of THINLENS / NONE
SENTINEL = 0x7FC0DEAD              # a NaN's bits: no call writes it


def refused_host_calls(cam):
    """the failures of the six host single-item calls, camera_reverse_ray and ghost_pairs() on a camera whose last update failed: each
    must return ZOIC_ERR_NOT_UPDATED (camera_reverse_ray: 0) and leave its outputs, prefilled with SENTINEL, alone"""
    import ctypes as C
    from zoic_amd import _capi
    lib, h, bad = _capi.load(), cam._h, []
    o, d = _capi.Vec3(0.1, 0.1, -50.0), _capi.Vec3(-0.002, -0.002, 1.0)
    calls = {"zoic_trace_back_ray": lambda ps, f, j: lib.zoic_trace_back_ray(h, C.byref(o), C.byref(d), ps, C.byref(f)),
             "zoic_trace_back_ray_spectral": lambda ps, f, j: lib.zoic_trace_back_ray_spectral(h, C.byref(o), C.byref(d), 500.0, ps, C.byref(f)),
             "zoic_project_point": lambda ps, f, j: lib.zoic_project_point(h, C.byref(o), ps, C.byref(f)),
             "zoic_project_point_spectral": lambda ps, f, j: lib.zoic_project_point_spectral(h, C.byref(o), 500.0, ps, C.byref(f)),
             "zoic_trace_back_ray_jacobian": lambda ps, f, j: lib.zoic_trace_back_ray_jacobian(h, C.byref(o), C.byref(d), ps, C.byref(f), j),
             "zoic_trace_back_ray_jacobian_spectral": lambda ps, f, j: lib.zoic_trace_back_ray_jacobian_spectral(h, C.byref(o), C.byref(d), 500.0, ps, C.byref(f), j),
             "zoic_camera_reverse_ray": lambda ps, f, j: 9 if lib.zoic_camera_reverse_ray(h, C.byref(o), C.c_float(0.5), ps, C.cast(C.byref(f), C.POINTER(C.c_float))) == 0 else 0}
    for name, call in calls.items():
        out = np.full(2 + 1 + 12, SENTINEL, np.uint32)
        ps = C.cast(out.ctypes.data, C.POINTER(C.c_float))
        f = C.c_uint32.from_address(out.ctypes.data + 8)
        j = C.cast(out.ctypes.data + 12, C.POINTER(C.c_float))
        rc = call(ps, f, j)
        if rc != NOT_UPDATED or (out != SENTINEL).any():
            bad.append("%s on a camera that is not updated: status %d, %d words written" % (name, rc, (out != SENTINEL).sum()))
    if len(cam.ghost_pairs()) != 0:
        bad.append("ghost_pairs() lists pairs on a camera that is not updated")
    return bad


# ---- what the two modules do with a step --------------------------------------------------------------------------------------------
def same_tables(a, b):
    return all(np.array_equal(dc.bits(a[k]), dc.bits(b[k])) for k in a)


def twin_holds(fail, D, state, cam, B, H):
    """the getters and the six host single-item calls of a fresh tables-only camera brought straight to `state`: the same bits"""
    tw = D.twin(state)
    if state.model == RAYTRACED and not (same_tables(cam.dispersion(), tw.dispersion()) and same_tables(cam.coatings(), tw.coatings()) and np.array_equal(cam.ghost_pairs(), tw.ghost_pairs())):
        fail("the getters differ from the fresh twin's")
    for line in differing(H, host_backward(tw, B)):
        fail("against the fresh twin: " + line)
    tw.close()


def reverse_ray_holds(fail, cam, state, B, H):
    """camera_reverse_ray: the projection's bit 0 with the switch on, False with it off"""
    for q, f in list(zip(B["pts"], H["project"][1]))[::max(1, len(B["pts"]) // 8)]:
        got, want = cam.reverse_ray(q), bool(f & 1) and state.reverse
        if got != want:
            fail("reverse_ray(%s) is %s with the switch %s and project_point's flags %#x" % (q, got, state.reverse, f))


def take(drivers, oracle_lib, name, k, device, raytraced, dead, failed=None):
    """the note of step k of sequence `name`, the steps up to it taken first"""
    if name not in drivers:
        drivers[name] = Driver(oracle_lib, name, device)
    D = drivers[name]
    while D.done < k:
        j = D.done + 1
        st, state, got = D.update(j)
        note = D.seen[j] = dict(fail=[], state=state, step=st)
        if D.broken is not None:
            note["fail"].append("the checks of step %d raised: the camera's later steps are void" % D.broken)
            continue
        try:
            if got != st.status:
                note["fail"].append("the update gave %s, scripted %s" % (got, st.status))
            if got is not None:
                for line in refused_host_calls(D.cam):
                    note["fail"].append(line)
                if failed is not None:
                    failed(D, st, state, note)
            elif state.model == RAYTRACED:
                raytraced(D, st, state, note)
            else:
                dead(D, st, state, note)
        except Exception as e:  # noqa: BLE001
            import traceback
            note["fail"].append("raised %r\n%s" % (e, traceback.format_exc()))
            D.broken = j
    return D.seen[k]


def figures_of(note):
    """what a step's checks measured, without the arrays"""
    def small(v):
        return {k: small(x) for k, x in v.items() if not isinstance(x, np.ndarray)} if isinstance(v, dict) else v
    return small({k: v for k, v in note.items() if k not in ("fail", "state", "step")})

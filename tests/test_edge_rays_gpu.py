"""Decision-safe FAST on rays placed exactly at the edges where rounding decides (tests/edge_rays.py), on the MI355X.

Random samples reach a guard band for 0.001 ... 2 % of the rays, and the parity tests bound the flip *fraction*, so a guard that
is skipped somewhere passes them.  Here every ray is an edge ray: STRICT must be bit-exact to the oracle on all of them (batch
call and resident tile, both row layouts), FAST must decide every guarded edge (housing clips, the LUT's end) as the oracle does
(batch call, resident tile, the listed kernel's short and long path, the per-sample call, the spectral kernel), and
FAST_UNCHECKED -- the same arithmetic without the guard -- must flip a clear share of the same edges, each inside its
interface's band by the f64 restatement: the rays provably sit where rounding decides, and the bands cover FAST's error."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_FAST_UNCHECKED, PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import camera_params, hexagon_bokeh, ray_rng_states

import edge_rays as E
from device_cases import bits_f32 as _bits, delta as _delta
from fuzz_cameras import CUSTOM_LENS_5, CUSTOM_LENS_14, _oracle_spectral, perturbed_prescription
from spectral_ref import LAMBDA_D, spectral_iors

pytestmark = pytest.mark.gpu

DIR_RMSE_TOL = 1e-5
# FAST_UNCHECKED must flip at least this share of the guarded edge rays of every camera (measured 12.7 ... 35.6 %: DESIGN 4.3)
UNCHECKED_FLOOR = 0.05
MIN_RAYS = 1 << 15             # edge rays per camera (per wavelength set in the spectral test)
K_SHORT_LIST = 131072          # kolb_listed_body.hpp kShortList: longer lists take the listed kernel's long path
CUSTOM_KW = dict(sensorWidth=3.6, sensorHeight=2.4, focalLength=5.0, fStop=2.8, focalDistance=150.0)   # the default sensor
PERTURBED = [("tessar_f2.8.dat", 11, 0.1, "keep"), ("double_gauss_f2.0.dat", 12, 0.1, "drop"), ("petzval_f1.25.dat", 13, 0.1, "double"),
             ("triplet_f2.5.dat", 14, 0.1, "keep")]
PERTURBED_KW = dict(focalLength=5.0, fStop=2.8, focalDistance=120.0)


def _same(a, b):
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _camera(p, lens_text=None, image=None, abbe=None, precision=PRECISION_STRICT):
    cam = ZoicCamera(0)
    if lens_text is not None:
        cam.set_lens_text(lens_text)
    if abbe is not None:
        cam.set_abbe_numbers(abbe)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh() if image is None else image)
    cam.set_precision(precision)
    cam.update(**p)
    return cam


def _setups():
    """name -> (update() parameters, lens text, (stop, other-interface) edge floors of the generator).  C3 has no stop edge
    (tests/test_edge_rays_cpu.py STOP_UNREACHABLE); the hand-written lenses are held to the ray count only."""
    out = {}
    for cfg in ("C2", "C3", "C4", "C5"):
        out[cfg] = (camera_params(cfg), None, (0 if cfg == "C3" else 500, 200))
    out["C2-nolut"] = (dict(camera_params("C2"), kolbSamplingLUT=False), None, (500, 200))
    for name, text in (("custom5", CUSTOM_LENS_5), ("custom14", CUSTOM_LENS_14)):
        out[name] = (dict(CUSTOM_KW), text, (0, 0))
    return out


SETUPS = _setups()


def _tile_records(cam, s, rows):
    """the resident tile's answer for samples s (ray indices 0 ... n-1): (n, 8) zoic_ray records (rows=1) or (n, 21) AtCameraOutput
    rows (rows=0), in buckets of the tile's capacity"""
    n = len(s)
    cap = min(n, 65536)
    tile = cam.tile(cap, tid=5)
    tile.set_rows(rows)
    tile.set_inputs(1)
    out = np.zeros((n, 8 if rows else 21), np.float32)
    for a in range(0, n, cap):
        m = min(cap, n - a)
        tile.samples[:m] = s[a:a + m]
        tile.submit(m, a)
        tile.wait()
        out[a:a + m] = (tile.rays if rows else tile.outputs)[:m]
    tile.close()
    return out


def _record_flags(rec):
    return np.ascontiguousarray(rec[:, 7]).view(np.uint32) & 0xFF


def _check_camera(oracle_lib, name, p, text=None, floors=(0, 0)):
    """every assertion of the edge-ray contract on one camera; returns its tally line"""
    er = E.edge_rays(oracle_lib, p, lens_text=text, seed=7, stop_edges=floors[0], nonstop_edges=floors[1])
    s = er["samples"]
    n = len(s)
    assert n >= MIN_RAYS, (name, n, E.edge_tally(er))
    n_stop, n_other, _ = E.edge_counts(er)
    assert n_stop >= floors[0] and n_other >= floors[1], (name, E.edge_tally(er))
    guarded = E.is_guarded(er)
    housing = er["kind"] == E.KINDS.index("housing")
    oc = E.oracle_camera(oracle_lib, p, text)
    before = oc.counters()
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, 0), threads=8)
    ocnt = oc.counters()
    orun = {k: ocnt[k] - before[k] for k in ocnt}         # this run's counts (ocnt: with the update's own TIR bumps)
    oc.close()

    # 1. STRICT: bit-exact on every edge ray, batch call and resident tile in both row layouts, counters included
    cam = _camera(p, text)
    got = cam.create_rays(s)
    assert np.array_equal(got["flags"], ref["flags"]), (name, int((got["flags"] != ref["flags"]).sum()))
    assert _same(got["planes"], ref["planes"]).all(), name
    assert cam.counters() == ocnt, (name, cam.counters(), ocnt)
    rec, cnt = _delta(cam, lambda: _tile_records(cam, s, 1))
    assert np.array_equal(_record_flags(rec), ref["flags"]), name
    assert _same(rec[:, 0:7].T, ref["planes"]).all(), name
    assert cnt == orun, (name, "tile, ray records", cnt, orun)
    rows, cnt = _delta(cam, lambda: _tile_records(cam, s, 0))
    assert _same(np.ascontiguousarray(rows[:, 0:6].T), ref["planes"][0:6]).all(), name
    assert np.array_equal(rows[:, 18], ref["weight"]), name
    assert cnt == orun, (name, "tile, AtCameraOutput rows", cnt, orun)
    cam.close()

    # 2. FAST: zero flips on guarded edges (batch call and resident tile), direction RMSE of the agreeing live rays
    cam = _camera(p, text, precision=PRECISION_FAST)
    if cam.info()["fastRunsStrict"]:
        cam.close()
        return None
    fast = cam.create_rays(s)
    frec = _tile_records(cam, s, 1)
    cam.close()
    fflip = fast["flags"] != ref["flags"]
    tflip = _record_flags(frec) != ref["flags"]
    labs = E.labels(er)
    bad = np.nonzero((fflip | tflip) & guarded)[0]
    live = ~fflip & (ref["weight"] != 0)
    dd = fast["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
    rmse = float(np.sqrt((dd ** 2).sum(0).mean())) if live.any() else 0.0
    assert rmse < DIR_RMSE_TOL, (name, rmse)

    # 3. UNCHECKED flips a clear share of the guarded edges; 4. every flip at a housing edge lies inside its band (f64 margin)
    cam = _camera(p, text, precision=PRECISION_FAST_UNCHECKED)
    unc = cam.create_rays(s)
    cam.close()
    uflip = (unc["flags"] != ref["flags"]) & guarded
    share = float(uflip.sum()) / max(1, int(guarded.sum()))
    hf = uflip & housing
    ratio = er["margin"][hf] / er["band"][hf]
    worst = {}
    for k in np.unique(labs[hf]):
        worst[str(k)] = float(ratio[labs[hf] == k].max())
    unguarded = {str(k): int(((fflip | tflip) & (labs == k)).sum()) for k in np.unique(labs[~guarded])}
    line = "%s: %d edge rays, edges %s | UNCHECKED flips %d of %d guarded (%.2f %%) | FAST flips on guarded %d, on unguarded %s | worst |m|/band %s | rmse %.2g" % (
        name, n, E.edge_tally(er), int(uflip.sum()), int(guarded.sum()), 100 * share, len(bad), unguarded, worst, rmse)
    print(line)
    assert share >= UNCHECKED_FLOOR, line
    assert (ratio < 1.0).all(), line
    # 2 (the verdict). FAST decides every guarded edge as the oracle does
    assert not len(bad), (name, "FAST flips on guarded edges (batch %d, tile %d)" % (int((fflip & guarded).sum()), int((tflip & guarded).sum())),
                          {str(k): int((labs[bad] == k).sum()) for k in np.unique(labs[bad])},
                          [(int(i), str(labs[i]), int(er["offset"][i]), int(ref["flags"][i]), int(fast["flags"][i]), float(er["margin"][i] / er["band"][i]))
                           for i in bad[:8]])
    return line


@pytest.mark.parametrize("name", list(SETUPS))
def test_edge_rays_strict_exact_fast_decision_safe(gpu, oracle_lib, name):
    p, text, floors = SETUPS[name]
    assert _check_camera(oracle_lib, name, p, text, floors) is not None, "%s: FAST runs STRICT on a camera it must serve" % name


@pytest.mark.parametrize("lens,seed,amount,surgery", PERTURBED, ids=["%s-%d-%s" % (a.split("_")[0], b, d) for a, b, c, d in PERTURBED])
def test_edge_rays_on_perturbed_prescriptions(gpu, oracle_lib, lens, seed, amount, surgery):
    """a machine-made lens of a fixed seed: STRICT-exact on its edges, decision-safe if inside FAST's domain (else skipped, counted
    by test_perturbed_prescriptions_run_fast)"""
    text = perturbed_prescription(lens, seed, amount, surgery).text
    line = _check_camera(oracle_lib, "%s/%d/%s" % (lens.split("_")[0], seed, surgery), dict(oracle_lib.DEFAULTS, **PERTURBED_KW), text, (0, 0))
    if line is None:
        pytest.skip("fastRunsStrict: FAST runs the STRICT kernels on this lens")


def test_perturbed_prescriptions_run_fast(gpu, oracle_lib):
    """at least 2 of the 4 machine-made lenses lie inside FAST's domain (their edge-ray test is not a skip)"""
    fast = 0
    for lens, seed, amount, surgery in PERTURBED:
        cam = _camera(dict(oracle_lib.DEFAULTS, **PERTURBED_KW), perturbed_prescription(lens, seed, amount, surgery).text, precision=PRECISION_FAST)
        fast += not cam.info()["fastRunsStrict"]
        cam.close()
    print("perturbed prescriptions: %d of %d run FAST" % (fast, len(PERTURBED)))
    assert fast >= 2


def test_listed_long_path_equals_short_path_on_edge_rays(gpu, oracle_lib):
    """One FAST launch of >= 2^18 edge rays, more than kShortList of them inside a guard band by the f64 margin (the listed
    kernel's long path), equals 4096-ray launches (short path), the resident kernel and per-sample calls bit for bit, counters
    included, and decides every guarded edge as the oracle does."""
    import torch
    p = camera_params("C4")
    er = E.edge_rays(oracle_lib, p, seed=11)
    # 2^18 rays: copies of the camera's edge rays, which differ in their ray index, i.e. in their retry streams only.  The list
    # length itself is not observable: that it exceeds kShortList is inferred from the f64 margins (almost every C4 edge ray lies
    # inside its band, worst |m| / band 0.5: the rays the main kernel cannot decide and lists).
    reps = -(-(1 << 18) // len(er["samples"]))
    s = np.ascontiguousarray(np.tile(er["samples"], (reps, 1)))
    n = len(s)
    housing = np.tile(er["kind"] == E.KINDS.index("housing"), reps)
    in_band = (housing & (np.tile(er["margin"], reps) < np.tile(er["band"], reps))) | np.tile(er["kind"] == E.KINDS.index("lut_end"), reps)
    guarded = np.tile(E.is_guarded(er), reps)
    assert int(in_band.sum()) > K_SHORT_LIST, int(in_band.sum())
    cam = _camera(p, precision=PRECISION_FAST)
    assert not cam.info()["fastRunsStrict"]
    dev = torch.device("cuda", 0)
    ts = torch.from_numpy(s).to(dev)
    whole, cw = _delta(cam, lambda: cam.create_rays(ts)["rays"].cpu().numpy())
    parts = []
    cp = {}
    for a in range(0, n, 4096):
        r, c = _delta(cam, lambda: cam.create_rays(ts[a:a + 4096].contiguous(), ray_index_base=a)["rays"].cpu().numpy())
        parts.append(r)
        cp = {k: cp.get(k, 0) + c[k] for k in c}
    parts = np.concatenate(parts)
    assert np.array_equal(_bits(parts), _bits(whole)), int((_bits(parts) != _bits(whole)).any(1).sum())
    assert cp == cw
    res, cr = _delta(cam, lambda: cam.create_rays_resident(ts).cpu().numpy())
    assert np.array_equal(_bits(res), _bits(whole)), int((_bits(res) != _bits(whole)).any(1).sum())
    assert cr == cw
    # per-sample calls: the first call of a fresh tid t draws from the batch stream of ray index (0xA7100000 | t) << 32
    pick = np.nonzero(guarded[:len(er["samples"])])[0]
    pick = pick[np.linspace(0, len(pick) - 1, 256).astype(int)]
    one_flags, one_states = [], []
    for t, k in enumerate(pick, start=1):
        one = cam.create_ray(*[float(v) for v in s[k]], tid=t)
        got = cam.create_rays(s[k:k + 1], ray_index_base=(0xA7100000 | t) << 32)
        have = np.array([one.origin.x, one.origin.y, one.origin.z, one.dir.x, one.dir.y, one.dir.z, one.weight[0]], np.float32)
        assert np.array_equal(_bits(have), _bits(got["planes"][:, 0])), (t, k)
        one_flags.append(int(got["flags"][0]))
        one_states.append(ray_rng_states(1, 1, (0xA7100000 | t) << 32)[0])
    cam.close()
    # ... and those rays, on those streams, decide as the oracle does (the per-sample call's flags are the one-ray launch's: equal bits)
    oc = E.oracle_camera(oracle_lib, p)
    one_ref = oc.create_rays(s[pick], rng_states=np.array(one_states, np.uint32))
    oc.close()
    assert np.array_equal(np.array(one_flags, np.uint8), one_ref["flags"]), int((np.array(one_flags) != one_ref["flags"]).sum())
    oc = E.oracle_camera(oracle_lib, p)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, 0), threads=8)
    oc.close()
    flips = (_record_flags(whole) != ref["flags"]) & guarded
    print("listed paths: %d rays, %d in a band by the f64 margin, %d guarded, FAST flips on guarded %d" % (n, in_band.sum(), guarded.sum(), flips.sum()))
    assert not flips.any()


@pytest.mark.parametrize("name", ["C2", "C5", "abbe-lens"])
def test_spectral_edge_rays(gpu, oracle_lib, name):
    """Edges generated at 400 nm, the d-line and 700 nm on each wavelength's index table: STRICT spectral is bit-exact to the
    oracle on them, FAST spectral decides every guarded one as the oracle does."""
    text, abbe = None, None
    if name == "abbe-lens":
        ml = perturbed_prescription("tessar_f2.8.dat", 21, 0.1, "keep", abbe=True)
        text, abbe = ml.text, ml.abbe
        p = dict(oracle_lib.DEFAULTS, **PERTURBED_KW)
    else:
        p = camera_params(name)
    cam = _camera(p, text, abbe=abbe)
    disp = cam.dispersion()
    assert disp["cauchy_b"].any()
    ss, lams, gs, ers = [], [], [], []
    for w in (np.float32(400.0), LAMBDA_D, np.float32(700.0)):
        er = E.edge_rays(oracle_lib, p, lens_text=text, ior=spectral_iors(disp["ior_d"], disp["cauchy_b"], w), seed=13, stop_edges=0,
                         nonstop_edges=0, min_rays=MIN_RAYS // 2, lut_screens=128)
        ss.append(er["samples"])
        lams.append(np.full(len(er["samples"]), w, np.float32))
        gs.append(E.is_guarded(er))
        ers.append(E.edge_tally(er))
    s, lam, guarded = np.concatenate(ss), np.concatenate(lams), np.concatenate(gs)
    n = len(s)
    assert n >= MIN_RAYS
    states = ray_rng_states(n, seed=2)
    got, cg = _delta(cam, lambda: cam.create_rays(s, rng_states=states, wavelengths=lam))
    ref, cr = _oracle_spectral(oracle_lib, p, disp, s, lam, states, lens_text=text)
    assert np.array_equal(got["flags"], ref["flags"])
    assert _same(got["planes"], ref["planes"]).all()
    assert cg == cr
    cam.close()
    fast = _camera(p, text, abbe=abbe, precision=PRECISION_FAST)
    assert not fast.info()["fastRunsStrict"]
    fr = fast.create_rays(s, rng_states=states, wavelengths=lam)
    fast.close()
    flips = (fr["flags"] != ref["flags"]) & guarded
    print("spectral %s: %d edge rays (%s), %d guarded, FAST flips on guarded %d" % (name, n, ers, guarded.sum(), flips.sum()))
    assert not flips.any()

"""Fuzz of the spectral kernels (zoic_create_rays_spectral_device) on cameras nobody drew: machine-made lenses (test_parity_gpu's
perturbed prescriptions and near-hemispherical rear elements) with a random V-number on every glass, random focal length, f-stop,
sensor, focus distance and LUT switch, now and then a random bokeh image.

  * STRICT against the oracle run on each wavelength's index table, wavelengths interleaved ray by ray: flags, planes (NaN equal to
    NaN) and counters identical; a camera the reference rejects is rejected with the same error class.
  * FAST against STRICT at wavelengths spread over all of 360 ... 830 nm: decision flips and the direction RMSE of agreeing live
    rays within the lens fuzz's bounds, worst case per wavelength band reported; a camera outside the FAST domain gives STRICT's bits.
  * hostile samples and hostile / boundary wavelengths in one batch: STRICT bit-exact to the oracle on the valid rows, the rejected
    rows zero records with flag 0x80 and no counts; FAST comes back with legal try counts."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, RAYTRACED, ZoicCamera
from zoic_amd.workloads import ray_rng_states

from device_cases import delta as _delta
from fuzz_cameras import (DIR_RMSE_TOL, EXAMPLE_CAMERA, EXAMPLE_LENSES, FLIP_TOL, HOSTILE_SAMPLES, LAMBDA_EDGES, LAMBDA_HOSTILE, WAVES, _oracle_spectral, bands, camera_params, camera_strategy, examples,
                          lens_args, lens_name, lens_strategy, perturbed_prescription, same_bits, update_both)

pytestmark = pytest.mark.gpu

LIVE_AT_ENDS = 100
BAND_NAMES = ["360-420", "420-500", "500-600", "600-700", "700-830"]


def _samples(rs, n, aspect=1.5):
    s = np.stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n) / aspect, rs.uniform(0, 1, n), rs.uniform(0, 1, n)], 1)
    return np.ascontiguousarray(s, np.float32)


def _camera(ml, img, precision=PRECISION_STRICT):
    cam = ZoicCamera(device=0)
    ml.load(cam)
    if img is not None:
        cam.set_bokeh_image(img)
    cam.set_precision(precision)
    return cam


def _new_tally():
    return dict(compared=0, rejected=0, strictOnly=0, rmse=0.0, flip=0.0, counts=set(), waves=set(), lamMin=np.inf, lamMax=-np.inf, live360=0, live830=0,
                band_rmse=[0.0] * len(BAND_NAMES), band_flip=[0.0] * len(BAND_NAMES))


def _print(name, t):
    print("%s: %d cameras compared (%d rejected alike, %d ran strict-only), worst direction RMSE %.3g, worst flip fraction %.3g, "
          "wavelengths %.6g ... %.6g nm (%d distinct; %d live rays compared at 360 nm, %d at 830 nm), interface counts %s"
          % (name, t["compared"], t["rejected"], t["strictOnly"], t["rmse"], t["flip"], t["lamMin"], t["lamMax"], len(t["waves"]), t["live360"],
             t["live830"], sorted(t["counts"])))
    if any(t["band_rmse"]) or any(t["band_flip"]):
        print("  per band (nm): " + ", ".join("%s: RMSE %.3g flip %.3g" % (b, r, f) for b, r, f in zip(BAND_NAMES, t["band_rmse"], t["band_flip"])))


def _draw(st):
    return st.tuples(lens_strategy(st, rear=True), camera_strategy(st), st.integers(0, 2 ** 20))


def _setup(oracle_lib, lens, draw, seed, kind):
    """the camera of one draw: (MachineLens, params, image, STRICT camera, error class or None)"""
    lens = lens_args(lens, sorted(draw.items()), seed)
    tag = "%s_%s_%d_%d" % (kind, lens_name(lens[0]), lens[1], seed)
    ml = perturbed_prescription(*lens, abbe=True)
    p, img = camera_params(draw, tag)
    p["lensDataPath"] = "mem:%s" % tag
    cam = _camera(ml, img)
    oc = oracle_lib.OracleCamera()
    oc.set_lens_text(ml.text)
    if img is not None:
        oc.set_bokeh_image(img)
    perr, oerr = update_both(cam, oc, p, oracle_lib)
    oc.close()
    assert perr == oerr, (ml.text, p, perr, oerr)
    return ml, p, img, cam, perr


def test_spectral_strict_and_fast_on_machine_made_cameras(gpu, oracle_lib):
    from hypothesis import example, given, settings, HealthCheck, strategies as st
    t = _new_tally()

    @settings(max_examples=examples("ZOIC_FUZZ_EXAMPLES_SPECTRAL", 40), deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(_draw(st))
    @example((EXAMPLE_LENSES[0], EXAMPLE_CAMERA, 1))
    @example((EXAMPLE_LENSES[1], EXAMPLE_CAMERA, 1))
    def run(arg):
        lens, draw, seed = arg
        ml, p, img, cam, err = _setup(oracle_lib, lens, draw, seed, "spec")
        if err is not None:
            t["rejected"] += 1
            cam.close()
            return
        disp = cam.dispersion()
        rs = np.random.RandomState(seed)
        n = 4096
        s = _samples(rs, n)
        lam = np.resize(WAVES, n)
        states = ray_rng_states(n, seed=seed)
        got, cg = _delta(cam, lambda: cam.create_rays(s, rng_states=states, wavelengths=lam))
        ref, cr = _oracle_spectral(oracle_lib, p, disp, s, lam, states, lens_text=ml.text, image=img)
        ctx = (ml.text, ml.abbe, p)
        assert np.array_equal(got["flags"], ref["flags"]), (ctx, int((got["flags"] != ref["flags"]).sum()))
        same = same_bits(got["planes"], ref["planes"])
        assert same.all(), (ctx, int((~same.all(0)).sum()))
        assert cg == cr, (ctx, cg, cr)
        t["live360"] += int(((lam == 360.0) & (got["weight"] != 0)).sum())
        t["live830"] += int(((lam == 830.0) & (got["weight"] != 0)).sum())
        t["compared"] += 1
        t["counts"].add(cam.info()["lensCount"])
        # FAST against STRICT, wavelengths over the whole range (both ends included)
        m = 8192
        s2 = _samples(rs, m)
        lam2 = rs.uniform(360.0, 830.0, m).astype(np.float32)
        lam2[: len(LAMBDA_EDGES)] = LAMBDA_EDGES
        t["waves"].update(np.unique(lam).tolist())
        t["lamMin"] = min(t["lamMin"], float(lam2.min()), float(lam.min()))
        t["lamMax"] = max(t["lamMax"], float(lam2.max()), float(lam.max()))
        a = cam.create_rays(s2, wavelengths=lam2)
        fast = _camera(ml, img, PRECISION_FAST)
        fast.update(**p)
        strictOnly = bool(fast.info()["fastRunsStrict"])
        t["strictOnly"] += strictOnly
        b = fast.create_rays(s2, wavelengths=lam2)
        agree = (a["flags"] == b["flags"]) & (a["weight"] == b["weight"])
        if strictOnly:
            assert np.array_equal(a["flags"], b["flags"]) and same_bits(a["planes"], b["planes"]).all(), ctx
        flip = 1.0 - float(agree.mean())
        t["flip"] = max(t["flip"], flip)
        live = agree & (a["weight"] != 0) & np.isfinite(a["dir"]).all(0)
        band = bands(lam2)
        for k in range(len(BAND_NAMES)):
            inb = band == k
            t["band_flip"][k] = max(t["band_flip"][k], 1.0 - float(agree[inb].mean()))
            lk = live & inb
            if lk.sum() > 50:
                dd = a["dir"][:, lk].astype(np.float64) - b["dir"][:, lk]
                t["band_rmse"][k] = max(t["band_rmse"][k], float(np.sqrt((dd ** 2).sum(0).mean())))
        assert flip < 20 * FLIP_TOL, (ctx, flip)
        if live.sum() > 100:
            dd = a["dir"][:, live].astype(np.float64) - b["dir"][:, live]
            rmse = float(np.sqrt((dd ** 2).sum(0).mean()))
            t["rmse"] = max(t["rmse"], rmse)
            assert rmse < DIR_RMSE_TOL, (ctx, rmse)
        fast.close()
        cam.close()
    run()
    _print("spectral fuzz", t)
    assert t["compared"] >= 20
    assert t["live360"] >= LIVE_AT_ENDS and t["live830"] >= LIVE_AT_ENDS    # rays really traced (and compared) at both ends of the range
    assert min(t["counts"]) <= 5 and max(t["counts"]) >= 14, sorted(t["counts"])


def test_spectral_hostile_samples_and_wavelengths(gpu, oracle_lib):
    from hypothesis import example, given, settings, HealthCheck, strategies as st
    t = _new_tally()

    @settings(max_examples=examples("ZOIC_FUZZ_EXAMPLES_SPECTRAL_HOSTILE", 24), deadline=None, suppress_health_check=list(HealthCheck),
              derandomize=True)
    @given(_draw(st), st.floats(0.1, 0.9))
    @example((EXAMPLE_LENSES[0], EXAMPLE_CAMERA, 1), 0.5)
    @example((EXAMPLE_LENSES[1], EXAMPLE_CAMERA, 1), 0.5)
    def run(arg, share):
        lens, draw, seed = arg
        ml, p, img, cam, err = _setup(oracle_lib, lens, draw, seed, "spechostile")
        if err is not None:
            t["rejected"] += 1
            cam.close()
            return
        disp = cam.dispersion()
        rs = np.random.RandomState(seed)
        n = 4096
        s = _samples(rs, n)
        hostile = rs.rand(n, 4) < share * 0.5
        s[hostile] = HOSTILE_SAMPLES[rs.randint(len(HOSTILE_SAMPLES), size=int(hostile.sum()))]
        lam = rs.uniform(360.0, 830.0, n).astype(np.float32)
        special = np.concatenate([LAMBDA_HOSTILE, LAMBDA_EDGES])
        odd = rs.rand(n) < share * 0.3
        lam[odd] = special[rs.randint(len(special), size=int(odd.sum()))]
        lam[: len(special)] = special
        valid = (lam >= 360.0) & (lam <= 830.0)
        assert not valid[: len(LAMBDA_HOSTILE)].any() and valid[len(LAMBDA_HOSTILE): len(special)].all()
        states = ray_rng_states(n, seed=seed)
        got, cg = _delta(cam, lambda: cam.create_rays(s, rng_states=states, wavelengths=lam))
        ref, cr = _oracle_spectral(oracle_lib, p, disp, s[valid], lam[valid], states[valid], lens_text=ml.text, image=img)
        ctx = (ml.text, ml.abbe, p)
        assert np.array_equal(got["flags"][valid], ref["flags"]), ctx
        same = same_bits(got["planes"][:, valid], ref["planes"])
        bad = np.nonzero(~same.all(0))[0]
        assert same.all(), (ctx, len(bad), s[valid][bad[:4]], lam[valid][bad[:4]])
        assert cg == cr, (ctx, cg, cr)                                  # the rejected rows count nowhere
        assert (got["flags"][~valid] == 0x80).all(), ctx
        assert not got["planes"][:, ~valid].view(np.uint32).any(), ctx   # +0.0 in all seven planes
        t["live360"] += int(((lam == 360.0) & (got["weight"] != 0)).sum())
        t["live830"] += int(((lam == 830.0) & (got["weight"] != 0)).sum())
        t["compared"] += 1
        t["counts"].add(cam.info()["lensCount"])
        t["waves"].update(np.unique(lam[valid]).tolist())
        t["lamMin"] = min(t["lamMin"], float(lam[valid].min()))
        t["lamMax"] = max(t["lamMax"], float(lam[valid].max()))
        cam.set_precision(PRECISION_FAST)
        t["strictOnly"] += bool(cam.info()["fastRunsStrict"])
        fast = cam.create_rays(s, rng_states=states, wavelengths=lam)
        assert (fast["tries"][valid] <= 26).all(), ctx
        assert (fast["flags"][~valid] == 0x80).all() and not fast["planes"][:, ~valid].view(np.uint32).any(), ctx
        cam.close()
    run()
    _print("spectral hostile fuzz", t)
    assert t["compared"] >= 20
    assert t["live360"] >= LIVE_AT_ENDS and t["live830"] >= LIVE_AT_ENDS    # rays really traced (and compared) at both ends of the range
    assert min(t["counts"]) <= 5 and max(t["counts"]) >= 14, sorted(t["counts"])

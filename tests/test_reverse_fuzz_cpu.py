"""Fuzz of the reverse projection (csrc/reverse.hpp) on cameras nobody drew: machine-made prescriptions (test_parity_gpu's perturbed
lenses: 5 ... 14 interfaces) behind random focal length, f-stop, sensor, focus distance and LUT switch.

  * without a GPU: the host build (host_drivers.reverse) recovers the screen samples of kolb_point_set's points
    within test_host_build_recovers_chief_ray_samples' bounds and equals the library's zoic_project_point; a camera outside the
    geometric domain flags every point kRevOutsideDomain; a lens with no unclipped chief ray gives an empty point set (counted);
  * on the GPU: zoic_project_points_device equals zoic_project_point bit for bit, flags included, on the accuracy set, wild points and
    an edge list (denormal and signed-zero coordinates, the front vertex, the z = 0 plane, infinite z, 1e38), batches of 1, 63, 64,
    65, 777 and all points."""
import zlib

import numpy as np
import pytest

from zoic_amd import RAYTRACED, ZoicCamera

from fuzz_cameras import EXAMPLE_CAMERA, EXAMPLE_LENSES, examples, lens_args, lens_name, lens_strategy, perturbed_prescription, rows_of
import host_drivers
from host_drivers import drive_reverse as _drive
from reverse_ref import OUTSIDE, kolb_point_set


@pytest.fixture(scope="module")
def driver():
    return host_drivers.reverse()


EXAMPLE = tuple(EXAMPLE_CAMERA[k] for k in ("focalLength", "fStop", "sensorWidth", "focalDistance", "kolbSamplingLUT"))


def _reason(f):
    return (np.asarray(f, np.int64) >> 8) & 15


def _draw(st):
    return st.tuples(lens_strategy(st), st.floats(2.0, 12.0, width=32), st.floats(1.25, 11.0, width=32), st.floats(1.0, 7.5, width=32),
                     st.floats(20.0, 2000.0, width=32), st.booleans())


def _camera(arg, device):
    """(camera, params, prescription text, inside the geometric domain) of one draw, or (None, params, text, None) if update rejects it"""
    key, focal, fstop, sensor_w, focus, lut = arg
    lens = lens_args(key, focal, fstop, sensor_w, focus, lut)
    ml = perturbed_prescription(*lens)
    p = dict(lensModel=RAYTRACED, lensDataPath="mem:rev_%s_%d" % (lens_name(lens[0]), lens[1]), focalLength=focal, fStop=fstop,
             sensorWidth=sensor_w, sensorHeight=sensor_w / 1.5, focalDistance=focus, kolbSamplingLUT=lut, useImage=False)
    cam = ZoicCamera(device=device)
    ml.load(cam)
    try:
        cam.update(**p)
    except Exception:  # noqa: BLE001
        cam.close()
        return None, p, ml.text, None
    i = cam.info()
    geometric = bool(i["focalLengthRatio"] > 0 and i["originShift"] < i["elements"][0, 1])
    return cam, p, ml.text, geometric


def _wild(seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (1024, 3)).astype(np.float32) * np.float32([50.0, 50.0, 200.0])


def test_reverse_fuzz_host_build(driver):  # noqa: F811
    from hypothesis import example, given, settings, HealthCheck, strategies as st
    t = dict(compared=0, rejected=0, outside=0, empty=0, points=0, worst=0.0, p99=0.0, counts=set())

    @settings(max_examples=examples("ZOIC_FUZZ_EXAMPLES_REVERSE", 40), deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(_draw(st))
    @example((EXAMPLE_LENSES[0],) + EXAMPLE)
    @example((EXAMPLE_LENSES[1],) + EXAMPLE)
    def run(arg):
        cam, p, text, geometric = _camera(arg, -1)
        if cam is None:
            t["rejected"] += 1
            return
        info = cam.info()
        ctx = (text, p)
        if not geometric:
            # outside the domain: every point, the axis included, is flagged kRevOutsideDomain and not projected
            assert info["fastRunsStrict"], ctx
            pts = np.concatenate([_wild(1)[:64], np.float32([[0, 0, -10], [0, 0, -1e4], [0.5, 0.5, -100]])])
            scr, fl = _drive(driver, cam, p, pts)
            assert (_reason(fl) == OUTSIDE).all() and not (fl & 1).any() and not scr.view(np.uint32).any(), ctx
            for q in pts[::8]:
                sx, sy, f = cam.project_point(q)
                assert _reason(f) == OUTSIDE and (sx, sy) == (0.0, 0.0), ctx
            t["outside"] += 1
            cam.close()
            return
        pts, s, depth = kolb_point_set(info, p["sensorWidth"], p["focalDistance"], grid=32)
        if len(pts) == 0:
            t["empty"] += 1
            cam.close()
            return
        scr, fl = _drive(driver, cam, p, pts)
        step = max(1, len(pts) // 256)
        lib = np.array([cam.project_point(q) for q in pts[::step]])
        assert np.array_equal(lib[:, :2].astype(np.float32).view(np.uint32), scr[::step].view(np.uint32)), ctx
        assert np.array_equal(lib[:, 2].astype(np.uint32), fl[::step]), ctx
        proj = (fl & 1) == 1
        assert proj.all(), (ctx, np.unique(_reason(fl[~proj]), return_counts=True))
        err = np.abs(scr.astype(np.float64) - s).max(1)
        assert err.max() <= 1e-5, (ctx, err.max())
        assert np.percentile(err, 99) <= 2e-6, (ctx, np.percentile(err, 99))
        assert not (fl & 2).any(), ctx   # the set's chief rays are unclipped: so is what the projection traced
        t["compared"] += 1
        t["points"] += len(pts)
        t["worst"] = max(t["worst"], float(err.max()))
        t["p99"] = max(t["p99"], float(np.percentile(err, 99)))
        t["counts"].add(info["lensCount"])
        cam.close()
    run()
    print("reverse fuzz (host build): %d cameras compared (%d rejected by update, %d outside the domain, %d with an empty point set), "
          "%d points, worst error %.3g, worst p99 %.3g, interface counts %s"
          % (t["compared"], t["rejected"], t["outside"], t["empty"], t["points"], t["worst"], t["p99"], sorted(t["counts"])))
    assert t["compared"] >= 20
    assert min(t["counts"]) <= 5 and max(t["counts"]) >= 14, sorted(t["counts"])


def _edges(info):
    """the extended edge list (records frame, Po = -Q): denormal and signed-zero coordinates, the front vertex, the z = 0 plane,
    infinite z, 1e38"""
    front = -float(info["elements"][:int(info["lensCount"]), 1].astype(np.float32).sum()) if info["lensCount"] else -1.0
    den, inf = 1e-40, np.inf
    e = [[0, 0, -10], [-0.0, -0.0, -10], [0.0, -0.0, -0.0], [-0.0, 0.0, 0.0], [den, 0, -10], [0, -den, -10], [den, den, -den], [-den, den, -100],
         [0, 0, -den], [0.1, 0.2, -den], [0, 0, front], [0.01, 0, front], [-0.3, 0.2, front], [0.5, 0.5, 0.0], [-1.0, 2.0, -0.0],
         [0, 0, -inf], [0, 0, inf], [0.1, 0.1, -inf], [1e38, 0, -1], [0, 1e38, -1e38], [1e38, 1e38, -1e38], [0, 0, -1e38], [0, 0, 1e38],
         [1e-30, 0, -1], [3e38, -3e38, -3e38], [np.nan, 0, -1], [0, 0, np.nan]]
    return np.array(e, np.float32)


@pytest.mark.gpu
def test_reverse_fuzz_batch_equals_host(gpu):
    import torch
    from hypothesis import example, given, settings, HealthCheck, strategies as st
    t = dict(compared=0, rejected=0, outside=0, empty=0, points=0, projected=0, counts=set())

    @settings(max_examples=examples("ZOIC_FUZZ_EXAMPLES_REVERSE_GPU", 24), deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(_draw(st))
    @example((EXAMPLE_LENSES[0],) + EXAMPLE)
    @example((EXAMPLE_LENSES[1],) + EXAMPLE)
    def run(arg):
        cam, p, text, geometric = _camera(arg, 0)
        if cam is None:
            t["rejected"] += 1
            return
        info = cam.info()
        acc = kolb_point_set(info, p["sensorWidth"], p["focalDistance"], grid=32)[0] if geometric else np.zeros((0, 3), np.float32)
        t["outside"] += not geometric
        t["empty"] += geometric and len(acc) == 0
        pts = np.ascontiguousarray(np.concatenate([acc, _wild(zlib.crc32(repr(arg).encode())), _edges(info)]), np.float32)
        host = np.array([cam.project_point(q) for q in pts])
        hs, hf = host[:, :2].astype(np.float32), host[:, 2].astype(np.uint32)
        ctx = (text, p)
        dev = torch.from_numpy(pts).to("cuda:0")
        for n in (1, 63, 64, 65, 777, len(pts)):
            for start in sorted({0, len(pts) - n}):
                scr, fl = cam.project_points(dev[start:start + n].contiguous())
                torch.cuda.synchronize()
                scr, fl = scr.cpu().numpy(), fl.cpu().numpy().astype(np.uint32)
                assert np.array_equal(scr.view(np.uint32), hs[start:start + n].view(np.uint32)), (ctx, n, start)
                assert np.array_equal(fl, hf[start:start + n]), (ctx, n, start)
        t["compared"] += 1
        t["points"] += len(pts)
        t["projected"] += int((hf & 1).sum())
        t["counts"].add(info["lensCount"])
        cam.close()
    run()
    print("reverse fuzz (device batch): %d cameras compared (%d rejected by update, %d outside the domain, %d with an empty accuracy set), "
          "%d points (%d projected), interface counts %s"
          % (t["compared"], t["rejected"], t["outside"], t["empty"], t["points"], t["projected"], sorted(t["counts"])))
    assert t["compared"] >= 20
    assert min(t["counts"]) <= 5 and max(t["counts"]) >= 14, sorted(t["counts"])


def test_point_set_of_a_lens_that_vignettes_its_whole_lattice():
    """kolb_point_set of a lens with no unclipped chief ray on its lattice is empty (it used to raise on the empty reduction)"""
    rows = [list(r) for r in rows_of("tessar_f2.8.dat")]
    rows[-1][-1] = 0.001                     # the rear element's aperture: every off-axis chief ray is clipped there
    cam = ZoicCamera(device=-1)
    cam.set_lens_text("".join("\t".join("%.6g" % v for v in r) + "\n" for r in rows))
    p = dict(lensModel=RAYTRACED, focalLength=5.0, fStop=4.0, sensorWidth=3.0, sensorHeight=2.0, focalDistance=200.0, kolbSamplingLUT=False,
             useImage=False)
    cam.update(**p)
    pts, s, depth = kolb_point_set(cam.info(), p["sensorWidth"], p["focalDistance"], grid=16)
    assert pts.shape == (0, 3) and s.shape == (0, 2) and depth.shape == (0,)
    cam.close()

"""Parity of the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

STRICT mode is held to bit-exactness (integer flags AND every f32 plane); FAST mode to the north-star tolerance
(direction RMSE < 1e-5 over rays with identical accept/try history and weight != 0, decision flips counted).
Full-size runs are checked through size-independent properties.
"""
import os

import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, RAYTRACED, THINLENS, ZoicCamera, lens_path
from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh, ray_count, ray_rng_states, synthetic_samples

from fuzz_cameras import CUSTOM_LENS_5, CUSTOM_LENS_14, HOSTILE_SAMPLES, REAR_ELEMENT_CASES, REAR_ELEMENT_LENS, perturbed_prescription
from device_cases import bits

pytestmark = pytest.mark.gpu

DIR_RMSE_TOL = 1e-5        # BASELINE.json north_star: "ray-direction RMSE <1e-5 vs CPU reference"
# Decision flips of FAST (the decision-safe mode: rays whose stop clip is too close to call are re-evaluated in STRICT
# arithmetic).  Measured 0 ... 4e-7 on C2-C5 (33 M rays each); the reference's own FMA / no-FMA builds flip 5e-6 ... 3e-4
# of the same rays (DESIGN.md "decision-safe fast mode").  A constant, not a knob.
FLIP_TOL = 5e-5
UNCHECKED_FLIP_TOL = 2e-3   # ZOIC_PRECISION_FAST_UNCHECKED (round 1's fast mode, kept for A/B): flips where the reference's own rounding decides


def make_pair(oracle_lib, cfg, **override):
    p = dict(camera_params(cfg), **override)
    cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
    if p.get("useImage"):
        img = hexagon_bokeh()
        cam.set_bokeh_image(img)
        oc.set_bokeh_image(img)
    cam.update(**p)
    oc.update(**p)
    return cam, oc


def slab(cfg, n, where=0.5):
    c = CONFIGS[cfg]
    base = int(c["width"] * int(c["height"] * where)) * c["spp"]
    return synthetic_samples(n, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base), base


def assert_bit_exact(got, ref):
    assert np.array_equal(got["flags"], ref["flags"])
    bad = (bits(got["planes"]) != bits(ref["planes"])).any(0)
    assert not bad.any(), "%d of %d rays differ" % (bad.sum(), bad.size)


@pytest.mark.parametrize("cfg,where", [("C1", 0.5), ("C2", 0.5), ("C2", 0.02), ("C3", 0.5), ("C4", 0.3), ("C5", 0.5), ("C5", 0.01)])
def test_strict_bit_exact_vs_oracle(gpu, oracle_lib, cfg, where):
    cam, oc = make_pair(oracle_lib, cfg)
    n = 1 << 17
    s, base = slab(cfg, n, where)
    got = cam.create_rays(s, ray_index_base=base)          # device derives the per-ray streams from (seed, index)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
    assert_bit_exact(got, ref)
    # counters: succes + vignetted == n; TIR equal (includes the LUT build's bumps)
    gc, occ = cam.counters(), oc.counters()
    assert gc == occ
    assert gc["succesRays"] + gc["vignettedRays"] == n


def test_strict_replays_the_sequential_reference_stream(gpu, oracle_lib):
    """The reference draws retries from ONE global xorshift stream in ray order (single thread).  The oracle run in
    that mode records the stream state at each ray's first retry; feeding those states to the GPU reproduces the
    sequential run exactly for every ray whose retries are contiguous in the stream (all of them: a ray finishes its
    retries before the next ray starts)."""
    cam, oc = make_pair(oracle_lib, "C2")
    n = 1 << 16
    s, base = slab("C2", n, 0.4)
    ref = oc.create_rays(s, want_first_retry_states=True)   # global sequential stream, continues after the LUT build
    states = ref["first_retry_states"].copy()
    states[(states == 0).all(1)] = (1, 2, 3, 4)             # never-retried rays: any non-zero state
    got = cam.create_rays(s, rng_states=states)
    assert_bit_exact(got, ref)
    assert 0.1 < float((ref["flags"] & 1).mean()) < 0.9


def test_retry_dead_ray_whose_draw_is_the_disk_centre(gpu, oracle_lib):
    """Retry-dead rays are completed by the finish kernel, which only steps their retry stream -- unless a
    draw is exactly (0.5, 0.5): the concentric-disk sample is then NaN, a NaN ray passes every comparison of the reference's
    trace, and the ray is a SUCCESS with NaN origin / direction at that try.  Probability 2e-15 per draw, so it is staged:
    streams built to produce 0x80000000 twice at their first draw (xor128 run backwards), and at their fifth."""
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT
    cam, oc = make_pair(oracle_lib, "C2")
    n = 1 << 15
    s, base = slab("C2", n, 0.02)                      # top rows of the TESSAR frame: off-axis, retries cannot reach the rear element
    states = ray_rng_states(n, 1, base)
    plain = oc.create_rays(s, rng_states=states)
    dead = np.flatnonzero((plain["weight"] == 0) & (((plain["flags"] >> 1) & 31) == 26))
    assert dead.size > 2000
    first = np.array([0, 0x04809010, 0x12345678, 0x80001000], np.uint32)   # outputs 1, 2 = 0x80000000, 0x80000000

    def step_back(st):                                  # the xorshift128 state one draw earlier
        x1, y1, z1, w1 = (int(v) for v in st)
        w0 = z1
        u = w1 ^ w0 ^ (w0 >> 19)                       # = t ^ (t >> 8)
        t = u ^ (u >> 8) ^ (u >> 16) ^ (u >> 24)
        x0 = (t ^ (t << 11) ^ (t << 22)) & 0xffffffff
        return np.array([x0, x1, y1, w0], np.uint32)
    fifth = first
    for _ in range(8):                                  # four draws = eight numbers earlier
        fifth = step_back(fifth)
    states[dead[0::9]] = first
    states[dead[4::9]] = fifth
    ref = oc.create_rays(s, rng_states=states)
    hit1, hit5 = dead[0::9], dead[4::9]
    assert (ref["weight"][hit1] == 1).all() and (((ref["flags"][hit1] >> 1) & 31) == 1).all() and np.isnan(ref["planes"][3:6, hit1]).all()
    assert (ref["weight"][hit5] == 1).all() and (((ref["flags"][hit5] >> 1) & 31) == 5).all()
    for mode in (PRECISION_STRICT, PRECISION_FAST):
        cam.set_precision(mode)
        got = cam.create_rays(s, rng_states=states)
        assert np.array_equal(got["flags"], ref["flags"])
        assert np.array_equal(got["weight"], ref["weight"])
        g, r = got["planes"], ref["planes"]
        assert np.array_equal(np.isnan(g), np.isnan(r))
        if mode == PRECISION_STRICT:
            assert ((bits(g) == bits(r)) | np.isnan(r)).all()


@pytest.mark.parametrize("kw", [
    dict(kolbSamplingLUT=False),                                        # naive sampling over the rear element, zoic.cpp:1873-1888
    dict(exposureControl=1.5), dict(exposureControl=-2.0),              # zoic.cpp:1981-1987
    dict(focalDistance=23.0, fStop=2.8),
    dict(sensorWidth=7.9),                                              # radial distance beyond the LUT (fenced UB) -> flag bit 6
])
def test_strict_parameter_variants(gpu, oracle_lib, kw):
    cam, oc = make_pair(oracle_lib, "C2", **kw)
    n = 1 << 15
    s, base = slab("C2", n, 0.05)
    got = cam.create_rays(s, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base))
    assert_bit_exact(got, ref)
    if "sensorWidth" in kw:
        assert (got["flags"] & 64).any() and np.all(got["weight"][(got["flags"] & 64) != 0] == 0)


def test_strict_thinlens_variants(gpu, oracle_lib):
    n = 1 << 15
    for kw in (dict(opticalVignettingDistance=5.0), dict(opticalVignettingDistance=5.0, opticalVignettingRadius=0.4),
               dict(useDof=False), dict(useImage=True, bokehPath="procedural:hexagon256", opticalVignettingDistance=3.0),
               dict(exposureControl=0.7),
               dict(opticalVignettingDistance=30.0),                       # nearly every ray runs out of tries
               dict(opticalVignettingDistance=1.0, exposureControl=-0.5),  # a few retries per wave: refill next to fresh rays
               dict(useImage=True, bokehPath="procedural:hexagon256", opticalVignettingDistance=12.0, opticalVignettingRadius=1.5)):
        cam, oc = make_pair(oracle_lib, "C1", **kw)
        s, base = slab("C1", n, 0.7)
        got = cam.create_rays(s, ray_index_base=base)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base))
        assert_bit_exact(got, ref)


def test_strict_edge_inputs(gpu, oracle_lib):
    """Empty batch, a single ray, sx=sy=0 (d==0: the reference's --begin() UB, fenced), lens centre (NaN sample),
    u=1.0 lens samples, ragged batch sizes that do not fill a wave."""
    cam, oc = make_pair(oracle_lib, "C3")
    got = cam.create_rays(np.zeros((0, 4), np.float32))
    assert got["planes"].shape == (7, 0)
    edge = np.array([[0, 0, 0.25, 0.75], [0, 0, 0.5, 0.5], [0.3, -0.2, 0.5, 0.5], [1, 0.5625, 1.0, 1.0],
                     [-1, -0.5625, 0.0, 0.0], [0.999, 0.0, 1.0, 0.0]], np.float32)
    for n in (1, 6, 63, 65, 257):
        s = np.resize(edge, (n, 4)).astype(np.float32)
        st = ray_rng_states(n, 1, 0)
        got = cam.create_rays(s)
        ref = oc.create_rays(s, rng_states=st)
        assert np.array_equal(got["flags"], ref["flags"])
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))   # NaN payloads may differ; NaN-ness may not
        assert same.all()


def test_arnold_layout_adapter(gpu, oracle_lib):
    """AtCameraInput (28 B) -> AtCameraOutput (84 B): origin/dir/weight, dOdy/dDdy only for retried rays."""
    cam, oc = make_pair(oracle_lib, "C2")
    n = 4096
    s, base = slab("C2", n, 0.1)
    inp = np.zeros((n, 7), np.float32)
    inp[:, 0], inp[:, 1], inp[:, 4], inp[:, 5] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    out = cam.create_rays_arnold(inp, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base))
    assert np.array_equal(bits(out[:, 0:3].T.copy()), bits(ref["origin"]))
    assert np.array_equal(bits(out[:, 3:6].T.copy()), bits(ref["dir"]))
    assert np.array_equal(out[:, 18], ref["weight"]) and np.array_equal(out[:, 19], ref["weight"])
    retried = (ref["flags"] & 1) != 0
    assert np.array_equal(out[retried, 9:12], out[retried, 0:3]) and np.array_equal(out[retried, 15:18], out[retried, 3:6])
    assert not out[~retried, 9:12].any() and not out[~retried, 15:18].any()
    assert not out[:, 6:9].any() and not out[:, 12:15].any()
    one = cam.create_ray(float(s[7, 0]), float(s[7, 1]), float(s[7, 2]), float(s[7, 3]))
    # n==1 uses ray index 0's stream, so compare a first-try ray only
    k = int(np.argmax(~retried))
    one = cam.create_ray(*[float(v) for v in s[k]])
    assert (one.dir.x, one.dir.y, one.dir.z) == tuple(float(v) for v in ref["dir"][:, k])


@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_fast_mode_within_tolerance(gpu, oracle_lib, cfg):
    cam, oc = make_pair(oracle_lib, cfg)
    cam.set_precision(PRECISION_FAST)
    assert not cam.info()["fastRunsStrict"]      # the benchmark configurations are inside the fast modes' domain
    n = 1 << 18
    s, base = slab(cfg, n, 0.35)
    got = cam.create_rays(s, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base), threads=8)
    same = got["flags"] == ref["flags"]
    flip = 1.0 - float(same.mean())
    live = same & (ref["weight"] != 0)
    assert live.sum() > 1000 or cfg == "C5"
    if live.any():
        dd = got["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
        do = got["origin"][:, live].astype(np.float64) - ref["origin"][:, live]
        rmse = float(np.sqrt((dd ** 2).sum(0).mean()))
        ormse = float(np.sqrt((do ** 2).sum(0).mean()))
        assert rmse < DIR_RMSE_TOL, rmse
        assert ormse < 1e-4, ormse                  # hit position on the front element, cm
        assert np.array_equal(got["weight"][live], ref["weight"][live])
    assert flip < FLIP_TOL, flip
    # weight statistics agree even across flipped rays
    assert abs(float((got["weight"] == 0).mean()) - float((ref["weight"] == 0).mean())) < 2e-3


def test_results_do_not_depend_on_batch_split(gpu, oracle_lib):
    """A frame split over launches (or GPUs) gives the same rays: streams are keyed by the global ray index."""
    cam, _ = make_pair(oracle_lib, "C2")
    for mode in (PRECISION_STRICT, PRECISION_FAST):
        cam.set_precision(mode)
        n = 100000
        s, base = slab("C2", n, 0.2)
        whole = cam.create_rays(s, ray_index_base=base)
        parts = [cam.create_rays(s[a:b], ray_index_base=base + a) for a, b in ((0, 1), (1, 33333), (33333, 99999), (99999, n))]
        cat = np.concatenate([p["planes"] for p in parts], axis=1)
        assert np.array_equal(bits(cat), bits(whole["planes"]))
        assert np.array_equal(np.concatenate([p["flags"] for p in parts]), whole["flags"])


def test_device_sample_generator_matches_numpy(gpu):
    import torch
    cam = ZoicCamera(0).update(**camera_params("C1"))
    for cfg, base in (("C3", 0), ("C3", 132710400 - 4096), ("C5", (1 << 32) + 12345)):
        c = CONFIGS[cfg]
        n = 4096
        d = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base)
        torch.cuda.synchronize()
        h = synthetic_samples(n, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base)
        assert np.array_equal(bits(d.cpu().numpy()), bits(h))


def test_full_frame_properties_c3(gpu, oracle_lib):
    """BASELINE size (C3: 132.7 M samples), fast and strict, through size-independent properties: every ray
    accounted for once; accepted rays leave the front element (z=0 side) with unit direction heading to -z;
    zero-weight fraction near the oracle's on a sample; device-torch path == host-numpy path on a slab."""
    import torch
    c = CONFIGS["C3"]
    n = ray_count("C3")
    cam, oc = make_pair(oracle_lib, "C3")
    samples = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1)
    for mode in (PRECISION_STRICT, PRECISION_FAST):
        cam.set_precision(mode)
        cam.reset_counters()
        out = cam.create_rays(samples)
        torch.cuda.synchronize()
        cnt = cam.counters()
        assert cnt["succesRays"] + cnt["vignettedRays"] == n
        w, fl = out["weight"], out["flags"]
        assert int((w == 0).sum().item()) == cnt["vignettedRays"]
        assert bool(((w == 0) == ((fl >> 1) == 26)).all().item())
        live = w != 0
        d = out["dir"][:, live]
        nrm = (d * d).sum(0).sqrt()
        assert float((nrm - 1).abs().max().item()) < 2e-5
        assert bool((d[2] < 0).all().item())
        assert float(out["origin"][2][live].abs().max().item()) < 1.0     # front surface sag: |z| well under 1 cm
        k = 1 << 16
        base = 77 * c["width"] * c["spp"]
        host = cam.create_rays(samples[base:base + k].cpu().numpy(), ray_index_base=base)
        assert np.array_equal(bits(host["planes"]), bits(out["planes"][:, base:base + k].cpu().numpy()))
        if mode == PRECISION_STRICT:
            ref = oc.create_rays(samples[base:base + k].cpu().numpy(), rng_states=ray_rng_states(k, 1, base), threads=8)
            assert_bit_exact(host, ref)
    frac = cnt["vignettedRays"] / n
    assert 0.0 <= frac < 0.01


@pytest.mark.parametrize("cfg,frac_lo,frac_hi", [("C2", 0.10, 0.30), ("C4", 0.0, 0.01), ("C5", 0.0, 1.0)])
def test_full_frame_properties_other_configs(gpu, oracle_lib, cfg, frac_lo, frac_hi):
    """The other Kolb configs at their full BASELINE sizes (C2 16.6 M, C4 265 M, C5 2.1 G samples = 102 GB of samples +
    records), fast and strict: every ray accounted for once, zero weight <=> out of tries, accepted rays have unit
    direction heading to -z, a slab of the device result equals the host-buffer path bit for bit and (strict) the oracle."""
    import torch
    c = CONFIGS[cfg]
    n = ray_count(cfg)
    cam, oc = make_pair(oracle_lib, cfg)
    samples = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1)
    out = dict(rays=torch.empty((n, 8), dtype=torch.float32, device="cuda"))
    for mode in (PRECISION_STRICT, PRECISION_FAST):
        cam.set_precision(mode)
        cam.reset_counters()
        res = cam.create_rays(samples, out=out)
        torch.cuda.synchronize()
        cnt = cam.counters()
        assert cnt["succesRays"] + cnt["vignettedRays"] == n
        rays = res["rays"]
        w = rays[:, 6]
        fl = rays[:, 7].view(torch.int32)
        tries, lut_miss = (fl >> 1) & 31, (fl >> 6) & 1
        zero = w == 0
        assert int(zero.sum().item()) == cnt["vignettedRays"]
        assert bool((zero == ((tries == 26) | (lut_miss == 1))).all().item())   # out of tries (zoic.cpp:1951) or outside the LUT
        del tries, lut_miss, fl
        step = max(1, n // (1 << 26))            # unit-direction check on a strided sample of at most 64 M rays
        sub = rays[::step]
        live = sub[:, 6] != 0
        d = sub[:, 3:6][live]
        assert float(((d * d).sum(1).sqrt() - 1).abs().max().item()) < 2e-5
        assert bool((d[:, 2] < 0).all().item())
        del d, live, sub, zero
        k = 1 << 15
        base = (c["height"] // 3) * c["width"] * c["spp"]
        host = cam.create_rays(samples[base:base + k].cpu().numpy(), ray_index_base=base)
        dev = rays[base:base + k].cpu().numpy()
        assert np.array_equal(bits(host["planes"]), bits(np.ascontiguousarray(dev[:, :7].T)))
        if mode == PRECISION_STRICT:
            ref = oc.create_rays(samples[base:base + k].cpu().numpy(), rng_states=ray_rng_states(k, 1, base), threads=8)
            assert_bit_exact(host, ref)
    assert frac_lo <= cnt["vignettedRays"] / n <= frac_hi


@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_gpu_lut_build_equals_host_lut_build(gpu, oracle_lib, monkeypatch, cfg):
    """node_update builds the exit-pupil LUT on the GPU by default -- every thread jumps into the reference's ONE sequential
    xorshift128 stream (GF(2) matrix powers), draws, traces and boxes its probes (lut_build.hip); ZOIC_LUT_HOST=2 is round 1's
    build (GPU traces, host draws and replay), =1 the host loop.  All three must give the oracle's table, its TIR count and
    leave the stream where the reference leaves it (the next retry of tid 0 draws from there)."""
    p = dict(camera_params(cfg), useImage=False)
    oc = oracle_lib.OracleCamera().update(**p)
    n = 2000
    s, _ = slab(cfg, 8 * n, 0.3)
    s = s[::8]
    ref = oc.create_rays(s)                                  # the sequential global stream, continuing after the LUT build
    for mode in (None, "2", "1"):
        if mode is None:
            monkeypatch.delenv("ZOIC_LUT_HOST", raising=False)
        else:
            monkeypatch.setenv("ZOIC_LUT_HOST", mode)
        cam = ZoicCamera(0).update(**p)
        assert np.array_equal(bits(cam.info()["lutBoxes"]), bits(oc.lut()[1])), mode
        assert cam.counters()["totalInternalReflection"] == oc_tir_after_update(oracle_lib, p), mode
        got = [cam.create_ray(*[float(v) for v in row], tid=0) for row in s[:400]]
        d = np.array([(o.dir.x, o.dir.y, o.dir.z) for o in got], np.float32)
        assert np.array_equal(bits(d.T.copy()), bits(ref["dir"][:, :400])), mode
        cam.close()


def oc_tir_after_update(oracle_lib, p):
    return oracle_lib.OracleCamera().update(**p).counters()["totalInternalReflection"]


@pytest.mark.parametrize("shape,kind", [((256, 256), "hexagon"), ((200, 300), "random"), ((37, 5), "random"), ((6, 4), "flat"),
                                        ((64, 64), "sparse"), ((1024, 1024), "random")])
def test_gpu_cdf_build_equals_host_and_oracle(gpu, oracle_lib, monkeypatch, shape, kind):
    """bokehProbability on the GPU (bokeh_cdf.hip: row-parallel sequential sums + LDS bitonic sorts) gives the oracle's
    tables bit for bit, including the tie rule on flat / mostly-black images; ZOIC_CDF_HOST=1 keeps the build on the host."""
    h, w = shape
    rs = np.random.RandomState(h * 1000 + w)
    if kind == "hexagon":
        img = hexagon_bokeh(h)
    elif kind == "flat":
        img = np.ones((h, w, 3), np.float32)
    elif kind == "sparse":
        lum = (rs.rand(h, w) > 0.9).astype(np.float32) * rs.rand(h, w).astype(np.float32)
        lum[3] = 0
        img = np.repeat(lum[:, :, None], 3, 2)
    else:
        img = rs.rand(h, w, 3).astype(np.float32)
    kw = dict(lensModel=THINLENS, useImage=True, bokehPath="mem:%s%dx%d" % (kind, h, w))
    g = ZoicCamera(0); g.set_bokeh_image(img); g.update(**kw)
    monkeypatch.setenv("ZOIC_CDF_HOST", "1")
    c = ZoicCamera(0); c.set_bokeh_image(img); c.update(**kw)
    oc = oracle_lib.OracleCamera(); oc.set_bokeh_image(img); oc.update(**kw)
    a, b, o = g.bokeh_tables(), c.bokeh_tables(), oc.bokeh_tables()
    for k in ("rowIndices", "columnIndices"):
        assert np.array_equal(a[k], o[k]), k
        assert np.array_equal(b[k], o[k]), k
    for k in ("cdfRow", "cdfColumn"):
        assert np.array_equal(bits(a[k]), bits(o[k])), k
        assert np.array_equal(bits(b[k]), bits(o[k])), k
    # and rays drawn through those tables agree with the oracle (thin lens + image-based bokeh)
    n = 4096
    s, base = slab("C1", n, 0.4)
    got = g.create_rays(s, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base))
    assert_bit_exact(got, ref)


# the first 10 rows of CUSTOM_LENS_14 (back focus on the last one), and the same with its cemented doublet made a singlet
CUSTOM_LENS_10 = ("80.0\t3.0\t1.6\t40.0\n200.0\t1.0\t0.0\t40.0\n60.0\t3.0\t1.65\t36.0\n150.0\t1.0\t0.0\t36.0\n45.0\t4.0\t1.7\t30.0\n"
                  "90.0\t6.0\t0.0\t28.0\n0\t6.0\t0\t20.0\n-90.0\t2.0\t1.6\t24.0\n120.0\t4.0\t1.7\t26.0\n-60.0\t60.0\t0.0\t26.0\n")
CUSTOM_LENS_9 = ("80.0\t3.0\t1.6\t40.0\n200.0\t1.0\t0.0\t40.0\n60.0\t3.0\t1.65\t36.0\n150.0\t1.0\t0.0\t36.0\n45.0\t4.0\t1.7\t30.0\n"
                 "90.0\t6.0\t0.0\t28.0\n0\t6.0\t0\t20.0\n-90.0\t6.0\t1.6\t24.0\n-60.0\t60.0\t0.0\t26.0\n")


@pytest.mark.parametrize("text,count", [(CUSTOM_LENS_5, 5), (CUSTOM_LENS_14, 14), (CUSTOM_LENS_9, 9), (CUSTOM_LENS_10, 10)])
def test_generic_interface_count_path(gpu, oracle_lib, text, count):
    """Lenses whose interface count has no unrolled instantiation (not 7..12) run the rolled generic trace; 9 and 10 are
    the unrolled instantiations no shipped prescription reaches.  Strict must be bit-exact, fast within tolerance."""
    kw = dict(focalLength=5.0, fStop=2.8, focalDistance=150.0)
    cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
    cam.set_lens_text(text)
    oc.set_lens_text(text)
    cam.update(**kw)
    oc.update(**kw)
    assert cam.info()["lensCount"] == count
    n = 1 << 16
    s, base = slab("C2", n, 0.45)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base), threads=8)
    got = cam.create_rays(s, ray_index_base=base)
    assert_bit_exact(got, ref)
    assert float((ref["weight"] != 0).mean()) > 0.05
    cam.set_precision(PRECISION_FAST)
    fast = cam.create_rays(s, ray_index_base=base)
    same = fast["flags"] == ref["flags"]
    live = same & (ref["weight"] != 0)
    dd = fast["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
    assert float(np.sqrt((dd ** 2).sum(0).mean())) < DIR_RMSE_TOL
    assert 1.0 - float(same.mean()) < FLIP_TOL


@pytest.mark.parametrize("shape,kind", [((256, 256), "falloff"), ((150, 200), "falloff"), ((64, 48), "spots"), ((256, 256), "spots"),
                                        ((512, 512), "hexagon"), ((700, 1000), "falloff"), ((1100, 300), "spots")])
@pytest.mark.parametrize("cells_on_host", [False, True])
def test_bokeh_cell_records_exact_on_dense_cells(gpu, oracle_lib, monkeypatch, shape, kind, cells_on_host):
    """The cell-record sampler (one LDS record + one global record per lens sample) must return std::upper_bound's pixel
    for every sample: images whose sorted CDFs crowd many entries into one cell (exponential falloff; a few bright spots on
    a dim noisy background) exercise the exceptional path, and lens samples of exactly 0, 1.0, > 1, < 0 and NaN the
    out-of-range path.  Strict mode, bit-exact against the oracle (zoic.cpp:420-485)."""
    if cells_on_host:
        if shape not in ((150, 200), (1100, 300)):
            pytest.skip("host build of the records: two shapes are enough")
        monkeypatch.setenv("ZOIC_CELLS_HOST", "1")      # the records are built by the host loop instead of the GPU kernel
    h, w = shape
    rs = np.random.RandomState(11)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    if kind == "hexagon":
        lum = hexagon_bokeh(h)[:, :, 0].astype(np.float32)
    elif kind == "falloff":
        lum = np.exp(-((xx - w / 2) ** 2 + (yy - h / 2) ** 2) / (0.02 * w * h)).astype(np.float32) + 1e-6 * rs.rand(h, w).astype(np.float32)
    else:
        lum = 1e-4 * rs.rand(h, w).astype(np.float32)
        for _ in range(5):
            lum[rs.randint(h), rs.randint(w)] = 1.0
    img = np.repeat(lum[:, :, None], 3, axis=2).astype(np.float32)
    p = dict(camera_params("C3"), bokehPath="mem:%s%dx%d" % (kind, w, h))
    cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
    cam.set_bokeh_image(img); oc.set_bokeh_image(img)
    cam.update(**p); oc.update(**p)
    n = 1 << 16
    s, base = slab("C3", n, 0.5)
    s = s.copy()
    s[:64, 2] = np.resize(np.array([0.0, 1.0, 1.5, -0.25, np.nan, 0.99999994, 1e-30, 0.5], np.float32), 64)
    s[:64, 3] = np.resize(np.array([0.5, 0.0, 1.0, np.nan, 0.25, -1.0, 0.99999994, 2.0, 0.75], np.float32), 64)
    got = cam.create_rays(s, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
    assert np.array_equal(got["flags"], ref["flags"])
    g, r = got["planes"], ref["planes"]
    same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
    assert same.all(), "%d rays differ" % (~same.all(0)).sum()


@pytest.mark.parametrize("shape,path", [((2048, 2048), "GPU CDF build + cell records at the row limit (32 KB of row records in LDS)"),
                                        ((512, 4096), "GPU CDF build + cell records at the column limit"),
                                        ((2049, 64), "2049 rows: no cell records, the 16-ary pyramid sampler"),
                                        ((64, 4100), "4100 columns: host CDF build, no pyramid -- the reference's binary search")])
def test_bokeh_image_size_envelope(gpu, oracle_lib, shape, path):
    """bokehProbability / bokehSample (zoic.cpp:222-485) have no size limit; the device paths change with the image size
    (bokeh_cdf.hip up to 4096 x 4096, cell records up to 2048 rows x 4096 columns, the pyramid up to 4096 entries per CDF).
    Every path must sample the reference's pixel: strict, bit-exact against the oracle, Kolb and thin lens."""
    h, w = shape
    rs = np.random.RandomState(h * 7 + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    lum = (np.exp(-(((xx - 0.4 * w) / (0.3 * w)) ** 2 + ((yy - 0.55 * h) / (0.25 * h)) ** 2)).astype(np.float32)
           + np.float32(0.05) * rs.rand(h, w).astype(np.float32))
    lum[: h // 8] = 0.0                                   # a zero-luminance band: the plateau at the end of every CDF
    img = np.repeat(lum[:, :, None], 3, axis=2).astype(np.float32)
    n = 1 << 15
    for cfg, kw in (("C3", {}), ("C1", dict(useImage=True, opticalVignettingDistance=3.0))):
        p = dict(camera_params(cfg), bokehPath="mem:envelope%dx%d" % (w, h), **kw)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        cam.set_bokeh_image(img); oc.set_bokeh_image(img)
        cam.update(**p); oc.update(**p)
        s, base = slab("C3", n, 0.45)
        got = cam.create_rays(s, ray_index_base=base)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
        assert np.array_equal(got["flags"], ref["flags"]), (cfg, path)
        same = (bits(got["planes"]) == bits(ref["planes"])) | (np.isnan(got["planes"]) & np.isnan(ref["planes"]))
        assert same.all(), "%s, %s: %d rays differ" % (cfg, path, (~same.all(0)).sum())
        assert cam.counters() == oc.counters()
        cam.close()


@pytest.mark.parametrize("radius,back", REAR_ELEMENT_CASES)
def test_retry_dead_shortcut_with_a_near_hemispherical_rear_element(gpu, oracle_lib, radius, back):
    """The retry-dead shortcut (tables.hpp KolbTable::retry*) bounds the lens points that can reach the rear element's
    vertex-side cap.  raySphereIntersection takes ONE signed root and never rejects t < 0 (zoic.cpp:986): with a rear
    element whose housing radius is close to |R| and a short back focus an oblique retry can land on the OPPOSITE cap of
    the sphere and pass interface 0.  The per-ray bound retryMaxD (lens_system.cpp fill_table) leaves such rays to their 26
    draws; with sensorWidth 7 the frame reaches far off axis.  Strict, bit-exact, every slab of the frame."""
    text = REAR_ELEMENT_LENS.format(r=abs(radius), radius=radius, back=back)
    for focal in (5.0, 10.0):
        p = dict(camera_params("C2"), sensorWidth=7.0, sensorHeight=7.0 / 1.5, focalLength=focal, lensDataPath="mem:rear%g_%g" % (radius, back))
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        cam.set_lens_text(text); oc.set_lens_text(text)
        perr = oerr = None
        try:
            cam.update(**p)
        except Exception as e:  # noqa: BLE001
            perr = getattr(e, "status_name", type(e).__name__).replace("ZOIC_ERR_", "")
        try:
            oc.update(**p)
        except oracle_lib.OracleError as e:
            oerr = oracle_lib.ERR_NAMES[e.code]
        assert perr == oerr, (p, perr, oerr)
        if perr is not None:
            continue
        n = 1 << 15
        for where in (0.02, 0.2, 0.5, 0.93):
            s, base = slab("C2", n, where)
            got = cam.create_rays(s, ray_index_base=base)
            ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
            assert np.array_equal(got["flags"], ref["flags"]), (radius, back, focal, where)
            same = (bits(got["planes"]) == bits(ref["planes"])) | (np.isnan(got["planes"]) & np.isnan(ref["planes"]))
            assert same.all(), (radius, back, focal, where, int((~same.all(0)).sum()))
        assert cam.counters() == oc.counters()
        cam.close()


# statistics of the TRUE reference (zoic.cpp built against a stub ai.h in the survey container) on
# 480 x 270 x 4 samples with the pinned camera parameters: (zero-weight fraction, retried fraction)
REFERENCE_PROBE_STATS = {"C2": (0.19, 0.24), "C3": (0.0007, 0.16), "C4": (0.0, 0.10), "C5": (0.79, 0.86)}


@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5"])
def test_ray_statistics_match_the_reference_probe(gpu, cfg):
    """The one corroboration of the whole retry loop that does not go through the oracle: the fractions of zero-weight and
    of retried rays the real reference produced for these cameras (figures quoted to two digits: +-0.5 % absolute).
    tests/test_oracle_assumptions.py shows what these figures pin (the both-component translation of a retry, zoic.cpp:1933:
    translated in x only, TESSAR's 19 % zero-weight would be 0) and what no statistic can (the order of a retry's two draws)."""
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT
    cam = ZoicCamera(0)
    if CONFIGS[cfg]["bokeh"]:
        cam.set_bokeh_image(hexagon_bokeh())
    cam.update(**camera_params(cfg))
    n = 480 * 270 * 4
    s = synthetic_samples(n, 480, 270, 4, seed=1)
    zero_ref, retried_ref = REFERENCE_PROBE_STATS[cfg]
    for mode in (PRECISION_STRICT, PRECISION_FAST):
        cam.set_precision(mode)
        got = cam.create_rays(s)
        zero, retried = float((got["weight"] == 0).mean()), float((got["flags"] & 1).mean())
        assert abs(zero - zero_ref) < 0.005 and abs(retried - retried_ref) < 0.005, (cfg, mode, zero, retried)
    cam.close()


def test_launches_in_flight_on_several_streams(gpu):
    """One camera, 24 batches of different sizes queued round-robin on 4 HIP streams before anything is waited for: every
    launch owns its set of work cursors (a ring of 64), so each batch must come out exactly as when it runs alone."""
    import torch
    cam = ZoicCamera(0)
    cam.set_bokeh_image(hexagon_bokeh())
    cam.update(**camera_params("C3"))
    c = CONFIGS["C3"]
    sizes = [200_000 + 37_111 * i for i in range(24)]
    bases = [c["width"] * 700 * c["spp"] + 1_000_003 * i for i in range(24)]
    samples = [cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=3, ray_index_base=b) for n, b in zip(sizes, bases)]
    torch.cuda.synchronize()
    alone = []
    for s, b in zip(samples, bases):
        alone.append(cam.create_rays(s, ray_index_base=b)["rays"].clone())
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    outs = [dict(rays=torch.empty((n, 8), dtype=torch.float32, device="cuda")) for n in sizes]
    for i, (s, b) in enumerate(zip(samples, bases)):
        cam.create_rays(s, ray_index_base=b, out=outs[i], stream=streams[i % 4].cuda_stream)
    torch.cuda.synchronize()
    for i in range(24):
        assert torch.equal(outs[i]["rays"].view(torch.int32), alone[i].view(torch.int32)), "batch %d differs" % i


@pytest.mark.parametrize("lens,focal,fstop", [("mori_f2.8.dat", 5.0, 2.8), ("mori_f2.8.dat", 3.0, 5.6),
                                             ("triplet_f2.5.dat", 5.0, 2.5), ("triplet_f2.5.dat", 3.5, 8.0)])
@pytest.mark.parametrize("lut", [True, False])
def test_strict_bit_exact_other_prescriptions(gpu, oracle_lib, lens, focal, fstop, lut):
    """The shipped prescriptions the BASELINE configs do not use (7 and 11 interfaces; F_1.6_PETZVAL and F_5.0_TELEPHOTO have no stop
    row and are rejected with ZOIC_ERR_NO_APERTURE, tests/test_host_tables.py), with and without the exit-pupil LUT, strict mode,
    bit-exact vs the oracle."""
    p = dict(camera_params("C2"), lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, kolbSamplingLUT=lut)
    cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
    cam.update(**p); oc.update(**p)
    n = 1 << 15
    for where in (0.5, 0.04):
        s, base = slab("C2", n, where)
        got = cam.create_rays(s, ray_index_base=base)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
        assert_bit_exact(got, ref)
    assert cam.counters() == oc.counters()


@pytest.mark.parametrize("kw", [dict(opticalVignettingDistance=2.0), dict(opticalVignettingDistance=8.0, opticalVignettingRadius=1.2),
                                dict(useImage=True, bokehPath="procedural:hexagon256", opticalVignettingDistance=4.0)])
def test_fast_mode_thinlens_vignetting_within_tolerance(gpu, oracle_lib, kw):
    """The fast arithmetic of the thin-lens refill kernel (rsq normalisation, f32 disk mapping, v_sqrt in the vignetting
    test): same tolerances as the Kolb fast mode -- direction RMSE < 1e-5 on rays whose accept/reject history agrees,
    decision flips below FLIP_TOL."""
    cam, oc = make_pair(oracle_lib, "C1", **kw)
    cam.set_precision(PRECISION_FAST)
    n = 1 << 17
    s, base = slab("C1", n, 0.6)
    got = cam.create_rays(s, ray_index_base=base)
    ref = oc.create_rays(s, rng_states=ray_rng_states(n, 1, base), threads=8)
    same = got["flags"] == ref["flags"]
    assert 1.0 - float(same.mean()) < FLIP_TOL
    live = same & (ref["weight"] != 0)
    assert live.sum() > 1000
    dd = got["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
    do = got["origin"][:, live].astype(np.float64) - ref["origin"][:, live]
    assert float(np.sqrt((dd ** 2).sum(0).mean())) < DIR_RMSE_TOL
    assert float(np.sqrt((do ** 2).sum(0).mean())) < 1e-5
    assert (ref["flags"] & 1).mean() > 0.05          # the retry loop really ran


def test_strict_parameter_fuzz(gpu, oracle_lib):
    """Machine-made cameras: every shipped prescription with a stop, focal length / f-stop / focus distance / sensor size /
    exposure / LUT and DOF switches drawn at random (both lens models), 4096 samples each from a random place of the frame.
    Strict mode must stay bit-identical to the oracle, counters included; parameter sets the reference aborts on must be
    rejected with the same error class on both sides."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES", "400")), deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), st.floats(1.0, 20.0, width=32), st.floats(1.0, 22.0, width=32), st.floats(20.0, 2000.0, width=32),
           st.floats(1.0, 7.0, width=32), st.floats(-2.0, 2.0, width=32), st.booleans(), st.booleans(), st.sampled_from([RAYTRACED, RAYTRACED, THINLENS]),
           st.floats(0.0, 6.0, width=32), st.floats(0.02, 0.98), st.integers(0, 2 ** 20))
    def run(lens, focal, fstop, focus, sensor_w, exposure, lut, dof, model, ov, where, seed):
        p = dict(lensModel=model, lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, focalDistance=focus, sensorWidth=sensor_w,
                 sensorHeight=sensor_w / 1.5, exposureControl=exposure, kolbSamplingLUT=lut, useDof=dof, opticalVignettingDistance=ov,
                 opticalVignettingRadius=1.0, useImage=False)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        perr = oerr = None
        try:
            cam.update(**p)
        except Exception as e:
            perr = getattr(e, "status_name", type(e).__name__).replace("ZOIC_ERR_", "")
        try:
            oc.update(**p)
        except oracle_lib.OracleError as e:
            oerr = oracle_lib.ERR_NAMES[e.code]
        assert perr == oerr, (p, perr, oerr)
        if perr is not None:
            return
        cam.set_seed(seed)
        n = 4096
        s, base = slab("C2", n, where)
        got = cam.create_rays(s, ray_index_base=base)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=seed, ray_index_base=base), threads=4)
        assert np.array_equal(got["flags"], ref["flags"]), p
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
        assert same.all(), (p, int((~same.all(0)).sum()))
        assert cam.counters() == oc.counters(), p
    run()


def test_fast_parameter_fuzz(gpu, oracle_lib):
    """The same machine-made cameras in FAST mode, 32 K samples each: direction RMSE < 1e-5 over the rays whose accept/try
    history agrees with the oracle, fewer than FLIP_TOL decision flips, zero-weight fractions within 0.5 %."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]
    worst = dict(rmse=0.0, flip=0.0, strictOnly=0, cameras=0)

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES_FAST", os.environ.get("ZOIC_FUZZ_EXAMPLES", "200"))), deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), st.floats(1.0, 20.0, width=32), st.floats(1.0, 22.0, width=32), st.floats(20.0, 2000.0, width=32),
           st.floats(1.0, 7.0, width=32), st.booleans(), st.sampled_from([RAYTRACED, RAYTRACED, RAYTRACED, THINLENS]), st.floats(0.0, 6.0, width=32),
           st.floats(0.02, 0.98))
    def run(lens, focal, fstop, focus, sensor_w, lut, model, ov, where):
        p = dict(lensModel=model, lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, focalDistance=focus, sensorWidth=sensor_w,
                 sensorHeight=sensor_w / 1.5, kolbSamplingLUT=lut, opticalVignettingDistance=ov, useImage=False)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        try:
            oc.update(**p)
        except oracle_lib.OracleError:
            return
        cam.update(**p)
        cam.set_precision(PRECISION_FAST)
        worst["strictOnly"] += bool(cam.info()["fastRunsStrict"])
        worst["cameras"] += 1
        n = 1 << 15
        s, base = slab("C2", n, where)
        got = cam.create_rays(s, ray_index_base=base)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
        same = got["flags"] == ref["flags"]
        flip = 1.0 - float(same.mean())
        assert flip < FLIP_TOL, (p, flip)
        assert abs(float((got["weight"] == 0).mean()) - float((ref["weight"] == 0).mean())) < 5e-3, p
        live = same & (ref["weight"] != 0)
        if live.sum() > 100:
            dd = got["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
            rmse = float(np.sqrt((dd ** 2).sum(0).mean()))
            assert rmse < DIR_RMSE_TOL, (p, rmse)
            worst["rmse"] = max(worst["rmse"], rmse)
        worst["flip"] = max(worst["flip"], flip)
    run()
    print("fast-mode fuzz: %d cameras (%d outside the fast modes' domain: they ran strict), worst direction RMSE %.3g, worst flip fraction %.3g"
          % (worst["cameras"], worst["strictOnly"], worst["rmse"], worst["flip"]))
    assert worst["strictOnly"] * 4 <= worst["cameras"]     # the shipped prescriptions are inside the domain but for odd focus settings


def test_wild_parameter_fuzz(gpu, oracle_lib):
    """Parameters far outside the UI's ranges (zoic.mtd) -- the reference checks none of them: focal lengths 0.2 ... 100,
    f-stops 0.3 ... 64, focus distances from inside the lens to 1e5, sensors 0.1 ... 12 wide, vignetting radii 0.1 ... 3,
    now and then a zero or a negative number.  Whatever node_update makes of them (negative apertures, NaN tables, a LUT
    of zeros) and whatever the rays then do, strict mode is bit-identical to the oracle, counters and error class included;
    the fast mode comes back with legal try counts."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]
    odd = st.sampled_from([0.0, -1.0, -5.0, 1e-6, 1e6])

    def wide(lo, hi):
        return st.one_of(st.floats(lo, hi, width=32), st.floats(lo, hi, width=32), st.floats(lo, hi, width=32), odd)

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES_WILD", os.environ.get("ZOIC_FUZZ_EXAMPLES", "100"))), deadline=None,
              suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), wide(0.25, 100.0), wide(0.3125, 64.0), wide(1.0, 1e5), wide(0.125, 12.0), wide(0.125, 3.0), wide(0.0, 50.0),
           st.floats(-6.0, 6.0, width=32), st.booleans(), st.booleans(), st.sampled_from([RAYTRACED, RAYTRACED, THINLENS]), st.floats(0.02, 0.98),
           st.integers(0, 2 ** 20))
    def run(lens, focal, fstop, focus, sensor_w, ovr, ov, exposure, lut, dof, model, where, seed):
        p = dict(lensModel=model, lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, focalDistance=focus, sensorWidth=sensor_w,
                 sensorHeight=sensor_w / 1.5, exposureControl=exposure, kolbSamplingLUT=lut, useDof=dof, opticalVignettingDistance=ov,
                 opticalVignettingRadius=ovr, useImage=False)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        perr = oerr = None
        try:
            cam.update(**p)
        except Exception as e:
            perr = getattr(e, "status_name", type(e).__name__).replace("ZOIC_ERR_", "")
        try:
            oc.update(**p)
        except oracle_lib.OracleError as e:
            oerr = oracle_lib.ERR_NAMES[e.code]
        assert perr == oerr, (p, perr, oerr)
        if perr is not None:
            return
        if model == RAYTRACED and lut:
            assert np.array_equal(bits(cam.info()["lutBoxes"]), bits(oc.lut()[1])), p
        cam.set_seed(seed)
        n = 4096
        s, base = slab("C2", n, where)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=seed, ray_index_base=base), threads=4)
        got = cam.create_rays(s, ray_index_base=base)
        assert np.array_equal(got["flags"], ref["flags"]), p
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
        assert same.all(), (p, int((~same.all(0)).sum()))
        assert cam.counters() == oc.counters(), p
        cam.set_precision(PRECISION_FAST)
        fast = cam.create_rays(s, ray_index_base=base)
        assert (fast["tries"] <= 26).all(), p
    run()


def test_hostile_sample_fuzz(gpu, oracle_lib):
    """Samples nobody should send, through cameras of every kind (both lens models, LUT on / off, bokeh image on / off, every
    shipped prescription with a stop): zeros of both signs, 0.5 (the disk mapping's 0/0), 1.0 and its neighbours, negative
    and > 1 lens samples, denormals, 1e30, infinities and NaNs in every component, mixed with ordinary samples in one
    batch.  The reference has no input checks: whatever its arithmetic makes of them (NaN rays that 'pass' every compare,
    LUT lookups off both ends -- fenced UB) the strict kernels must make too, bit for bit, counters included."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]
    special = HOSTILE_SAMPLES

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES_HOSTILE", os.environ.get("ZOIC_FUZZ_EXAMPLES", "80"))), deadline=None,
              suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), st.sampled_from([RAYTRACED, RAYTRACED, THINLENS]), st.booleans(), st.booleans(), st.floats(2.0, 12.0, width=32),
           st.floats(1.25, 11.0, width=32), st.floats(1.0, 7.5, width=32), st.floats(0.0, 4.0, width=32), st.integers(0, 2 ** 16), st.floats(0.1, 0.9))
    def run(lens, model, lut, image, focal, fstop, sensor_w, ov, seed, share):
        rs = np.random.RandomState(seed)
        p = dict(lensModel=model, lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, focalDistance=100.0, sensorWidth=sensor_w,
                 sensorHeight=sensor_w / 1.5, kolbSamplingLUT=lut, useImage=image, opticalVignettingDistance=ov, bokehPath="mem:hostile%d" % seed)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        if image:
            h, w = int(rs.randint(2, 40)), int(rs.randint(2, 40))
            img = np.repeat(rs.rand(h, w).astype(np.float32)[:, :, None], 3, axis=2)
            cam.set_bokeh_image(img); oc.set_bokeh_image(img)
        try:
            oc.update(**p)
        except oracle_lib.OracleError:
            return
        cam.update(**p)
        cam.set_seed(seed)
        n = 4096
        s, base = slab("C2", n, 0.5)
        s = s.copy()
        hostile = rs.rand(n, 4) < share * 0.5
        s[hostile] = special[rs.randint(len(special), size=int(hostile.sum()))]
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=seed, ray_index_base=base), threads=4)
        got = cam.create_rays(s, ray_index_base=base)
        assert np.array_equal(got["flags"], ref["flags"]), (p, np.nonzero(got["flags"] != ref["flags"])[0][:4], s[np.nonzero(got["flags"] != ref["flags"])[0][:4]])
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
        bad = np.nonzero(~same.all(0))[0]
        assert same.all(), (p, len(bad), s[bad[:4]], g[:, bad[:4]], r[:, bad[:4]])
        assert cam.counters() == oc.counters(), p
        # the same batch through the Arnold-layout entry point (28-byte AtCameraInput rows in, 84-byte AtCameraOutput rows out,
        # expanded on the GPU): origin / dir / weight as above, dOdy = origin and dDdy = dir for retried rays only (zoic.cpp:1974-1977)
        inp = np.zeros((n, 7), np.float32)
        inp[:, 0], inp[:, 1], inp[:, 4], inp[:, 5] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
        out = cam.create_rays_arnold(inp, ray_index_base=base)
        eq = lambda a, b: ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()   # noqa: E731
        assert eq(out[:, 0:3].T.copy(), ref["origin"]) and eq(out[:, 3:6].T.copy(), ref["dir"]), p
        assert eq(out[:, 18].copy(), ref["weight"]) and eq(out[:, 20].copy(), ref["weight"]), p
        retried = (ref["flags"] & 1) != 0
        assert eq(out[retried, 9:12].copy(), out[retried, 0:3].copy()) and eq(out[retried, 15:18].copy(), out[retried, 3:6].copy()), p
        assert not out[~retried, 9:12].any() and not out[~retried, 15:18].any() and not out[:, 6:9].any() and not out[:, 12:15].any(), p
        # the fast mode on the same batch: it must come back, every ray with a legal try count, and the ordinary samples of
        # the batch decided as the oracle decides them (hostile ones: NaN-ness of the direction as the oracle's)
        cam.set_precision(PRECISION_FAST)
        fast = cam.create_rays(s, ray_index_base=base)
        assert (fast["tries"] <= 26).all(), p
        plain = ~hostile.any(1)
        if plain.sum() > 200:
            assert float((fast["flags"][plain] != ref["flags"][plain]).mean()) < 40 * FLIP_TOL, p     # ~2000 rays: one flip is 5e-4
        assert np.array_equal(np.isnan(fast["dir"]).any(0), np.isnan(ref["dir"]).any(0)) or (fast["flags"] != ref["flags"]).any(), p
    run()


def test_perturbed_prescription_fuzz(gpu, oracle_lib):
    """Machine-made LENSES: a shipped prescription with every radius, thickness, index and aperture moved by up to
    +-25 %, sometimes with an element dropped or doubled (interface counts 5 ... 14: unrolled and rolled traces), behind
    random focal length / f-stop / LUT switch.  The geometry assumptions of the device shortcuts (retry-dead bound, dead
    pixels, guard bands, interface-0 search) must hold for lenses nobody drew: strict bit-identical to the oracle,
    counters included, the same error class when the reference aborts; fast mode: decisions as the oracle's (fewer than
    1e-3 flips of 8192 rays) and directions within a sanity bound (see below)."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES_LENS", os.environ.get("ZOIC_FUZZ_EXAMPLES", "150"))), deadline=None,
              suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), st.integers(0, 2 ** 16), st.floats(0.0, 0.25), st.sampled_from(["keep", "keep", "drop", "double"]),
           st.floats(2.0, 12.0, width=32), st.floats(1.25, 11.0, width=32), st.booleans(), st.floats(0.02, 0.98))
    def run(lens, seed, amount, surgery, focal, fstop, lut, where):
        text = perturbed_prescription(lens, seed, amount, surgery).text
        kw = dict(focalLength=focal, fStop=fstop, focalDistance=120.0, kolbSamplingLUT=lut)
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        cam.set_lens_text(text); oc.set_lens_text(text)
        perr = oerr = None
        try:
            cam.update(**kw)
        except Exception as e:
            perr = getattr(e, "status_name", type(e).__name__).replace("ZOIC_ERR_", "")
        try:
            oc.update(**kw)
        except oracle_lib.OracleError as e:
            oerr = oracle_lib.ERR_NAMES[e.code]
        assert perr == oerr, (text, kw, perr, oerr)
        if perr is not None:
            tally["rejected"] += 1
            return
        n = 8192
        s, base = slab("C2", n, where)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=4)
        got = cam.create_rays(s, ray_index_base=base)
        tally["compared"] += 1
        tally["alive"] += float((ref["weight"] != 0).mean())
        tally["retried"] += float(((ref["flags"] & 1) != 0).mean())
        tally["counts"].add(cam.info()["lensCount"])
        assert np.array_equal(got["flags"], ref["flags"]), (text, kw)
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
        assert same.all(), (text, kw, int((~same.all(0)).sum()))
        assert cam.counters() == oc.counters(), (text, kw)
        strictOnly = cam.info()["fastRunsStrict"]     # negative focal-length ratio or the sensor in front of the rear vertex: outside the FAST modes' domain (zoic_amd.h)
        i = cam.info()
        geometric = not (i["focalLengthRatio"] > 0 and i["originShift"] < i["elements"][0, 1])
        assert strictOnly or not geometric, (text, kw)      # the rest of strictOnly: node_update's self-check of the fast modes said no
        tally["selfCheck"] += bool(strictOnly and not geometric)
        tally["strictOnly"] += strictOnly
        cam.set_precision(PRECISION_FAST)
        fast = cam.create_rays(s, ray_index_base=base)
        agree = fast["flags"] == ref["flags"]
        if strictOnly:
            assert agree.all() and ((bits(fast["planes"]) == bits(r)) | (np.isnan(fast["planes"]) & np.isnan(r))).all(), (text, kw)
        assert 1.0 - float(agree.mean()) < 20 * FLIP_TOL, (text, kw, 1.0 - float(agree.mean()))   # 8192 rays: one flip is 1.2e-4
        live = agree & (ref["weight"] != 0) & np.isfinite(ref["dir"]).all(0)
        if live.sum() > 100:
            dd = fast["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
            rmse = float(np.sqrt((dd ** 2).sum(0).mean()))
            # 1e-5 is north_star's figure; node_update's self-check (capi.cpp fast_self_check) holds every camera to it on its
            # own 4096 probe rays and sends the others to STRICT (machine-made lenses can be badly conditioned: FAST takes
            # cos(i) from thc = sqrt(R^2 - d2), which cancels at grazing incidence -- 6e-5 on a fisheye with an element
            # removed).  This slab is another sample of the frame: three times the figure, worst case printed.
            assert rmse < 3 * DIR_RMSE_TOL, (text, kw, rmse)
            tally["rmse"] = max(tally["rmse"], rmse)
            tally["above"] += rmse >= DIR_RMSE_TOL
    tally = dict(rejected=0, compared=0, alive=0.0, retried=0.0, counts=set(), rmse=0.0, above=0, strictOnly=0, selfCheck=0)
    run()
    print("lens fuzz: %d cameras compared (%d rejected alike), mean live fraction %.2f, mean retried fraction %.2f, interface counts %s, worst fast-mode direction RMSE %.3g (%d cameras at or above 1e-5), %d cameras outside the fast modes' domain (%d of them by node_update's self-check)"
          % (tally["compared"], tally["rejected"], tally["alive"] / max(tally["compared"], 1), tally["retried"] / max(tally["compared"], 1), sorted(tally["counts"]), tally["rmse"], tally["above"], tally["strictOnly"], tally["selfCheck"]))
    assert tally["compared"] >= 10


@pytest.mark.parametrize("shape", [(7, 2), (16, 2), (2, 9), (5, 31)])
def test_retry_dead_bound_with_a_bokeh_image_that_is_not_square(gpu, oracle_lib, shape):
    """bokehSample centres columns with the image HEIGHT and rows with its WIDTH (zoic.cpp:441,466), so an image that is
    not square returns lens samples far outside the unit square (2 x 7 pixels: x in [-3, -2]).  The retry-dead shortcut
    bounds the disk the retries can sample; with the unit-square bound it declared PETZVAL rays dead that the reference
    gets through on their 2nd ... 12th try (found by test_bokeh_image_fuzz).  The bound is the image's own now
    (KolbTable::retryLensK)."""
    h, w = shape
    lum = np.random.RandomState(0).rand(h, w).astype(np.float32)
    img = np.repeat(lum[:, :, None], 3, axis=2).astype(np.float32)
    p = dict(lensModel=RAYTRACED, lensDataPath=lens_path("petzval_f1.25.dat"), focalLength=8.0, fStop=2.0, focalDistance=100.0, sensorWidth=3.0,
             sensorHeight=2.0, kolbSamplingLUT=True, useImage=True, bokehPath="mem:notsquare%dx%d" % (w, h))
    cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
    cam.set_bokeh_image(img); oc.set_bokeh_image(img)
    cam.update(**p); oc.update(**p)
    n = 1 << 15
    for where in (0.5, 0.1):
        s, base = slab("C3", n, where)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=1, ray_index_base=base), threads=8)
        got = cam.create_rays(s, ray_index_base=base)
        assert np.array_equal(got["flags"], ref["flags"])
        g, r = got["planes"], ref["planes"]
        assert ((bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))).all()
    assert cam.counters() == oc.counters()


def test_bokeh_image_fuzz(gpu, oracle_lib):
    """Machine-made bokeh images behind machine-made cameras (the IMAGE instantiations of the Kolb kernels and the thin-lens
    sampler): shape 2 ... 160 a side and not square, noise / a few bright spots / a falloff / black rows and columns,
    every shipped prescription with a stop, LUT on and off.  Strict mode must stay bit-identical to the oracle (flags, every
    plane, counters) -- in particular the retry search, which samples several draws of a ray's retry stream per round but
    may only count the ones the reference's loop would have drawn (zoic.cpp:1927-1947, 420-485); the decision-safe fast
    mode must keep its tolerance on the same camera."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    lenses = ["double_gauss_f2.0.dat", "tessar_f2.8.dat", "fisheye_muller_f4.0.dat", "petzval_f1.25.dat", "triplet_f2.5.dat", "mori_f2.8.dat"]

    @settings(max_examples=int(os.environ.get("ZOIC_FUZZ_EXAMPLES_IMAGE", os.environ.get("ZOIC_FUZZ_EXAMPLES", "60"))), deadline=None,
              suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.sampled_from(lenses), st.floats(2.0, 12.0, width=32), st.floats(1.25, 11.0, width=32), st.floats(1.0, 5.0, width=32), st.booleans(),
           st.sampled_from([RAYTRACED, RAYTRACED, RAYTRACED, THINLENS]), st.integers(2, 160), st.integers(2, 160),
           st.sampled_from(["noise", "spots", "falloff", "gaps"]), st.floats(0.02, 0.98), st.integers(0, 2 ** 20))
    def run(lens, focal, fstop, sensor_w, lut, model, h, w, kind, where, seed):
        rs = np.random.RandomState(seed & 0xffff)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        if kind == "noise":
            lum = rs.rand(h, w).astype(np.float32)
        elif kind == "spots":
            lum = 1e-4 * rs.rand(h, w).astype(np.float32)
            for _ in range(4):
                lum[rs.randint(h), rs.randint(w)] = 1.0
        elif kind == "falloff":
            lum = np.exp(-((xx - w / 2) ** 2 + (yy - h / 2) ** 2) / (0.03 * w * h + 1.0)).astype(np.float32) + 1e-6 * rs.rand(h, w).astype(np.float32)
        else:   # black rows and columns: zero-mass rows sort to the tail of the row CDF, zero pixels to the tail of a column CDF
            lum = rs.rand(h, w).astype(np.float32)
            lum[rs.rand(h) < 0.3, :] = 0.0
            lum[:, rs.rand(w) < 0.3] = 0.0
            if not (lum > 0).any():
                lum[h // 2, w // 2] = 1.0
        img = np.repeat(lum[:, :, None], 3, axis=2).astype(np.float32)
        p = dict(lensModel=model, lensDataPath=lens_path(lens), focalLength=focal, fStop=fstop, focalDistance=100.0, sensorWidth=sensor_w,
                 sensorHeight=sensor_w / 1.5, kolbSamplingLUT=lut, useImage=True, bokehPath="mem:fuzz%dx%d_%d" % (w, h, seed))
        cam, oc = ZoicCamera(0), oracle_lib.OracleCamera()
        cam.set_bokeh_image(img); oc.set_bokeh_image(img)
        try:
            oc.update(**p)
        except oracle_lib.OracleError:
            return
        cam.update(**p)
        ta, tb = cam.bokeh_tables(), oc.bokeh_tables()      # GPU CDF build (row sums, two descending sorts with ties, prefix sums)
        for k in ("rowIndices", "columnIndices"):
            assert np.array_equal(ta[k], tb[k]), (p, k)
        for k in ("cdfRow", "cdfColumn"):
            assert np.array_equal(bits(ta[k]), bits(tb[k])), (p, k)
        cam.set_seed(seed)
        n = 8192
        s, base = slab("C3", n, where)
        ref = oc.create_rays(s, rng_states=ray_rng_states(n, seed=seed, ray_index_base=base), threads=4)
        refCounters = oc.counters()
        got = cam.create_rays(s, ray_index_base=base)
        assert np.array_equal(got["flags"], ref["flags"]), p
        g, r = got["planes"], ref["planes"]
        same = (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))
        assert same.all(), (p, int((~same.all(0)).sum()))
        assert cam.counters() == refCounters, p
        if True:     # both models: the thin lens's fast sampler divides by the image size with v_rcp_f32
            cam.set_precision(PRECISION_FAST)
            fast = cam.create_rays(s, ray_index_base=base)
            agree = fast["flags"] == ref["flags"]
            assert 1.0 - float(agree.mean()) < 20 * FLIP_TOL, (p, 1.0 - float(agree.mean()))   # 8192 rays: one flip is 1.2e-4
            live = agree & (ref["weight"] != 0)
            if live.sum() > 100:
                dd = fast["dir"][:, live].astype(np.float64) - ref["dir"][:, live]
                assert float(np.sqrt((dd ** 2).sum(0).mean())) < DIR_RMSE_TOL, p
    run()


@pytest.mark.parametrize("cfg,extra", [("C5", {}), ("C1", dict(opticalVignettingDistance=3.0))])
def test_batches_beyond_2_to_31_samples_are_split(gpu, cfg, extra):
    """One call with 2^31 + 70 000 samples (103 GB of samples + records): the persistent kernels use 32-bit ray offsets, so
    the launcher splits the batch; every ray must be accounted for once and the rays either side of the split must equal
    the same rays computed as a small batch of their own (ray_index_base keys the streams)."""
    import torch
    import gc
    n = (1 << 31) + 70_000
    gc.collect()
    torch.cuda.empty_cache()                 # earlier tests' buffers sit in torch's caching allocator
    free, _ = torch.cuda.mem_get_info()
    if free < n * 48 + (8 << 30):
        pytest.skip("needs 111 GB of free HBM")
    c = CONFIGS[cfg]
    cam = ZoicCamera(0)
    cam.update(**dict(camera_params(cfg), **extra))
    cam.set_precision(PRECISION_FAST)
    samples = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=9)
    out = dict(rays=torch.empty((n, 8), dtype=torch.float32, device="cuda"))
    cam.reset_counters()
    cam.create_rays(samples, out=out)
    torch.cuda.synchronize()
    cnt = cam.counters()
    assert cnt["succesRays"] + cnt["vignettedRays"] == n
    lo, k = (1 << 31) - 50_000, 120_000                    # a window straddling the split
    ref = cam.create_rays(samples[lo:lo + k].clone(), ray_index_base=lo)["rays"]
    assert torch.equal(out["rays"][lo:lo + k].view(torch.int32), ref.view(torch.int32))
    tail = out["rays"][n - 1000:]
    assert bool(torch.isfinite(tail[:, 6]).all().item())   # the last rays were written


def test_listed_dead_pixels_do_not_depend_on_the_length_of_the_list(gpu):
    """A ray's bits must not depend on how a frame is cut.  The decision-safe FAST mode evaluates the rays it cannot decide in a
    second kernel with three evaluators: long work lists (> 131072 rays: batches + pool), short ones (tries side by side) and the resident
    kernel's one-ray loop.  A fisheye behind a sensor wider than its image circle has everything at once: 1-2 % of the rays listed, dead
    pixels (outside the exit-pupil LUT: all 27 tries are one) among them where the LUT ends -- their STRICT try-0 state must be what all
    three hand out.  One 12.6 M-ray launch (long list) == forty-eight 262144-ray launches (short lists) == tiles through the resident
    kernel, bit for bit, counters included."""
    import torch
    from zoic_amd import PRECISION_FAST, ZoicCamera
    p = dict(camera_params("C4"), sensorWidth=7.6, sensorHeight=7.6 / 1.5)
    cam = ZoicCamera(0)
    cam.update(**p)
    cam.set_precision(PRECISION_FAST)
    if cam.info()["fastRunsStrict"]:
        pytest.skip("the self-check sent this camera to STRICT: nothing is listed")
    W, H, spp = 1920, 1080, 6
    n = W * H * spp
    s = cam.generate_samples(n, W, H, spp, seed=3)
    cam.reset_counters()
    whole = cam.create_rays(s)["rays"].clone()
    torch.cuda.synchronize()
    c_whole = cam.counters()
    lut_miss = (whole[:, 7].view(torch.int32) & 64) != 0
    assert 0.02 < float(lut_miss.float().mean()) < 0.9, "the sensor must reach beyond the LUT"
    cam.reset_counters()
    piece = 1 << 18
    parts = torch.empty_like(whole)
    for a in range(0, n, piece):
        b = min(n, a + piece)
        parts[a:b] = cam.create_rays(s[a:b], ray_index_base=a)["rays"]
    torch.cuda.synchronize()
    c_parts = cam.counters()
    diff = (whole.view(torch.int32) != parts.view(torch.int32)).any(1)
    assert int(diff.sum()) == 0, (int(diff.sum()), torch.nonzero(diff)[:5].flatten().tolist())
    assert c_whole == c_parts
    # ... and the resident kernel's evaluator on a stretch that crosses the LUT's end
    rows = torch.nonzero(lut_miss)[:, 0]
    a = max(0, int(rows[len(rows) // 2]) - 30000)
    m = 60000
    host = s[a:a + m].cpu().numpy()
    inp = np.zeros((m, 7), np.float32)
    inp[:, 0], inp[:, 1], inp[:, 4], inp[:, 5] = host[:, 0], host[:, 1], host[:, 2], host[:, 3]
    out = cam.create_rays_tile(inp, ray_index_base=a, tid=0)
    ref = whole[a:a + m].cpu().numpy()
    assert np.array_equal(out[:, 0:6].view(np.uint32), ref[:, 0:6].view(np.uint32))
    assert np.array_equal(out[:, 18], ref[:, 6])
    cam.close()

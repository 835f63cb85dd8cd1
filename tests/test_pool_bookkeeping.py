"""The pool kernels' bookkeeping (kolb_pool_body.hpp): retry streams seeded at the pop from the launch's key, lane flags as wave masks.

None of it may change a ray: STRICT stays bit-identical to the oracle where most rays retry and where none does, with the streams
derived on the device and with the caller's states; a ray's FAST record does not depend on which pass, lane or launch evaluates it;
and a launch whose ray indices cross a multiple of 2^32 (where the streams' key changes inside the launch) gives the same rays.
"""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_FAST_UNCHECKED, PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh, ray_rng_states, synthetic_samples

from device_cases import bits

N_SLAB = 4096 + 63          # 64 whole batches and a partial one
N_SPLIT = 8192 + 65
# The retry-heavy slab: C3's camera, the first rows of a 3840 x 2880 lattice.  The 16:9 frame's own corner stops at 46 % retried rays; these
# rows lie further out on the sensor (54 % retried, 28 % out of tries: test_corner_slab_is_retry_heavy holds the oracle to that).
CORNER_LATTICE = (3840, 2880, 16)


def make_oracle(oracle_lib, cfg):
    p = camera_params(cfg)
    oc = oracle_lib.OracleCamera()
    if p.get("useImage"):
        oc.set_bokeh_image(hexagon_bokeh())
    oc.update(**p)
    return oc


def make_camera(cfg, precision):
    p = camera_params(cfg)
    cam = ZoicCamera(0)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    cam.update(**p)
    cam.set_precision(precision)
    if precision != PRECISION_STRICT:
        assert not cam.info()["fastRunsStrict"]
    return cam


def c3_slab(where):
    """(samples, ray index base) of the two C3 slabs."""
    if where == "corner":
        w, h, spp = CORNER_LATTICE
        return synthetic_samples(N_SLAB, w, h, spp, seed=1, ray_index_base=0), 0
    c = CONFIGS["C3"]
    base = (c["width"] * (c["height"] // 2) + c["width"] // 2) * c["spp"]
    return synthetic_samples(N_SLAB, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base), base


@pytest.fixture(scope="module")
def c3_reference(oracle_lib):
    """The oracle's rays and counters for the two slabs, computed once."""
    ref = {}
    for where in ("corner", "centre"):
        s, base = c3_slab(where)
        oc = make_oracle(oracle_lib, "C3")
        rays = oc.create_rays(s, rng_states=ray_rng_states(N_SLAB, 1, base), threads=8)
        ref[where] = (rays, oc.counters())
    return ref


def assert_bit_exact(got, ref):
    assert np.array_equal(got["flags"], ref["flags"])
    bad = (bits(got["planes"]) != bits(ref["planes"])).any(0)
    assert not bad.any(), "%d of %d rays differ" % (bad.sum(), bad.size)


def test_corner_slab_is_retry_heavy(c3_reference):
    rays, _ = c3_reference["corner"]
    retried = float((rays["flags"] & 1).mean())
    out_of_tries = float((rays["weight"] == 0).mean())
    print("corner slab: retried %.3f, out of tries %.3f" % (retried, out_of_tries))
    assert retried >= 0.5
    assert out_of_tries > 0.01
    centre, _ = c3_reference["centre"]
    assert float((centre["flags"] & 1).mean()) < 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("seeding", ["device", "states"])
@pytest.mark.parametrize("where", ["corner", "centre"])
def test_strict_retry_heavy_slab_bit_exact_with_counters(gpu, c3_reference, where, seeding):
    s, base = c3_slab(where)
    ref, ref_counters = c3_reference[where]
    cam = make_camera("C3", PRECISION_STRICT)
    if seeding == "device":
        got = cam.create_rays(s, ray_index_base=base)
    else:
        got = cam.create_rays(s, rng_states=ray_rng_states(N_SLAB, 1, base))
    assert_bit_exact(got, ref)
    assert cam.counters() == ref_counters


# (config, ray index base of the slab): rows where the first try fails often -- C3's and C4's frame corner, C2 (retry-dead rays and the
# two-level search) a tenth of the way down
SPLIT_CASES = [("C3", 0), ("C2", int(1920 * 108) * 8), ("C4", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [PRECISION_FAST, PRECISION_FAST_UNCHECKED], ids=["fast", "unchecked"])
@pytest.mark.parametrize("cfg,base", SPLIT_CASES, ids=[c for c, _ in SPLIT_CASES])
def test_fast_records_do_not_depend_on_the_launch_split(gpu, cfg, base, precision):
    """One launch against sub-launches of 1, 63, 64, 65 rays and the rest: pool order and pass composition differ, the records may not."""
    c = CONFIGS[cfg]
    s = synthetic_samples(N_SPLIT, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base)
    cam = make_camera(cfg, precision)
    whole = cam.create_rays(s, ray_index_base=base)
    retried = float((whole["flags"] & 1).mean())
    print("%s: retried %.3f" % (cfg, retried))
    assert retried > 0.05
    cuts = [0, 1, 64, 128, 193, N_SPLIT]
    parts = [cam.create_rays(s[a:b], ray_index_base=base + a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate([p["flags"] for p in parts]), whole["flags"])
    assert np.array_equal(bits(np.concatenate([p["planes"] for p in parts], axis=1)), bits(whole["planes"]))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["C3", "C2"])
def test_launch_across_a_multiple_of_2_to_32_ray_indices(gpu, oracle_lib, cfg):
    """4096 rays whose indices cross 2^32: the second half's retry streams have another key than the launch's."""
    n, half = 4096, 2048
    base = (1 << 32) - half
    if cfg == "C3":
        w, h, spp = CORNER_LATTICE
        s = synthetic_samples(n, w, h, spp, seed=1, ray_index_base=0)
    else:
        c = CONFIGS[cfg]
        s = synthetic_samples(n, c["width"], c["height"], c["spp"], seed=1, ray_index_base=SPLIT_CASES[1][1])
    states = ray_rng_states(n, 1, base)
    assert not np.array_equal(states[half:], ray_rng_states(half, 1, 0)), "the key changes at 2^32"
    oc = make_oracle(oracle_lib, cfg)
    ref = oc.create_rays(s, rng_states=states, threads=8)
    assert float((ref["flags"][half:] & 1).mean()) > 0.05      # rays past the boundary do draw from their streams
    cam = make_camera(cfg, PRECISION_STRICT)
    got = cam.create_rays(s, ray_index_base=base)
    assert_bit_exact(got, ref)
    assert cam.counters() == oc.counters()
    cam.set_precision(PRECISION_FAST)
    assert not cam.info()["fastRunsStrict"]
    whole = cam.create_rays(s, ray_index_base=base)
    lo, hi = cam.create_rays(s[:half], ray_index_base=base), cam.create_rays(s[half:], ray_index_base=base + half)
    assert np.array_equal(np.concatenate([lo["flags"], hi["flags"]]), whole["flags"])
    assert np.array_equal(bits(np.concatenate([lo["planes"], hi["planes"]], axis=1)), bits(whole["planes"]))

"""The edge-ray generator (tests/edge_rays.py) on its own, no GPU: its pairs are adjacent floats on which the oracle's first try
decides differently, it is deterministic, its housing edges lie on the clip by the f64 restatement (not on a sampler jump), and
it reaches every kind of edge the fast kernels guard, in numbers."""
import numpy as np
import pytest

from zoic_amd.workloads import camera_params, ray_rng_states

import edge_rays as E

CAMERAS = {"C2": ("C2", {}), "C2-nolut": ("C2", dict(kolbSamplingLUT=False)), "C3": ("C3", {}), "C4": ("C4", {}), "C5": ("C5", {})}
# C3 (DOUBLE_GAUSS behind the hexagon bokeh image): no first try is clipped at the stop.  The LUT scales the image's points into the
# exit pupil and the outer elements vignette first: of 3697 first-try failures of 20 000 random samples (9162 of 20 000 with lens
# samples within 0.02 of the square's edges) none was at the stop (interfaces 0, 7, 8, 9, 10 only).  Its stop has no edge to find.
STOP_UNREACHABLE = {"C3"}
_cache = {}


def _edges(oracle_lib, name, seed=1):
    if (name, seed) not in _cache:
        cfg, over = CAMERAS[name]
        _cache[(name, seed)] = E.edge_rays(oracle_lib, dict(camera_params(cfg), **over), seed=seed,
                                           stop_edges=0 if name in STOP_UNREACHABLE else 500)
    return _cache[(name, seed)]


@pytest.mark.parametrize("name", list(CAMERAS))
def test_pairs_are_adjacent_floats_that_the_oracle_decides_differently(oracle_lib, name):
    er = _edges(oracle_lib, name)
    a, b = er["pairs"][:, 0], er["pairs"][:, 1]
    diff = a != b
    assert (diff.sum(1) == 1).all(), "a pair differs in exactly one coordinate"
    x, y = np.abs(a[diff]), np.abs(b[diff])
    assert (np.nextafter(x, np.float32(np.inf)) == y).all(), "the two ends are adjacent floats"
    f = er["flags"]
    assert (((f[:, 0] ^ f[:, 1]) & 0x41) != 0).all(), "first-try outcome (bit 0) or LUT side (bit 6) differs"
    # the flags the generator recorded are the oracle's (a fresh camera, other streams: the first try does not draw)
    oc = E.oracle_camera(oracle_lib, dict(camera_params(CAMERAS[name][0]), **CAMERAS[name][1]))
    s = er["pairs"].reshape(-1, 4)
    again = oc.create_rays(s, rng_states=ray_rng_states(len(s), seed=9), threads=8)["flags"].reshape(-1, 2)
    assert np.array_equal(again & 0x41, f & 0x41)
    # every emitted ray is its edge's pair or an ulp neighbour of it on the pair's line
    assert len(er["samples"]) == len(er["edge"]) and np.array_equal(er["samples"][er["offset"] == 0], a)


def test_same_seed_same_rays(oracle_lib):
    p = camera_params("C5")
    one = E.edge_rays(oracle_lib, p, seed=4, screens=128, lut_screens=32)
    two = E.edge_rays(oracle_lib, p, seed=4, screens=128, lut_screens=32)
    other = E.edge_rays(oracle_lib, p, seed=5, screens=128, lut_screens=32)
    assert np.array_equal(one["samples"].view(np.uint32), two["samples"].view(np.uint32))
    for k in ("edge", "offset", "kind", "iface"):
        assert np.array_equal(one[k], two[k])
    assert np.array_equal(one["margin"], two["margin"], equal_nan=True)
    assert not np.array_equal(one["samples"], other["samples"])


@pytest.mark.parametrize("name", list(CAMERAS))
def test_housing_edges_lie_on_the_clip(oracle_lib, name):
    """the two ends of every housing(i) edge have an f64 margin within a few times the rounding the oracle's f32 trace can have
    there (eps |R| / housing at a near-planar interface, 64 eps of accumulated rounding elsewhere -- measured up to 1.1 x that):
    on the clip, not on a jump of the lens sampler"""
    er = _edges(oracle_lib, name)
    _, est = E.guard_bands(er["info"])
    floor = 64.0 * float(E.EPS)
    ends = (er["kind"] == E.KINDS.index("housing")) & np.isin(er["offset"], [0, 1])
    assert ends.any()
    scale = np.maximum(est[er["iface"][ends]], floor)
    ratio = er["margin"][ends] / scale
    print("%s: housing edge ends %d, worst |m| / max(est, 64 eps) %.3g, worst |m| / band %.3g" %
          (name, ends.sum(), ratio.max(), np.max(er["margin"][ends] / er["band"][ends])))
    assert ratio.max() < 4.0


@pytest.mark.parametrize("name,stop,nonstop,lut", [("C2", 500, 200, 200), ("C2-nolut", 500, 200, 0), ("C3", 0, 200, 200),
                                                   ("C4", 500, 200, 200), ("C5", 500, 200, 200)])
def test_coverage_floors(oracle_lib, name, stop, nonstop, lut):
    """distinct EDGES per kind: at the stop, at another interface (interface 0 on the camera without a LUT) and at the LUT's end;
    and 2^15 ... 2^16 edge rays per camera.  C3 has no stop edge at all (STOP_UNREACHABLE): its floor there is 0."""
    er = _edges(oracle_lib, name)
    n_stop, n_other, n_lut = E.edge_counts(er)
    print("%s: %d rays, %d edges (stop %d, other interfaces %d, LUT end %d): %s" % (name, len(er["samples"]), len(er["pairs"]),
                                                                                    n_stop, n_other, n_lut, E.edge_tally(er)))
    assert n_stop >= stop and n_other >= nonstop and n_lut >= lut
    if name == "C2-nolut":
        assert ((er["kind_e"] == E.KINDS.index("housing")) & (er["iface_e"] == 0)).sum() >= nonstop
    if name in STOP_UNREACHABLE:
        assert n_stop == 0, "a stop edge exists after all: give this camera its floor"
    assert (1 << 15) <= len(er["samples"]) <= (1 << 16)


def test_band_restatement_reads_the_source(oracle_lib):
    """the restated bands follow lens_system.hpp: every band at least the floor, a near-planar stop's band kGuardScaleFlat x its
    estimate"""
    c = E.guard_constants()
    assert c["scale"] > 0 and c["floor"] > 0 and c["min_rel"] > 0
    oc = E.oracle_camera(oracle_lib, camera_params("C4"))
    band, est = E.guard_bands(oc.lens_table())
    oc.close()
    assert (band >= c["floor"] * (1 - 1e-6)).all()
    stop = int(np.argmax(est))
    assert est[stop] > c["min_rel"]
    assert abs(band[stop] / (c["scale_flat"] * est[stop]) - 1.0) < 1e-3

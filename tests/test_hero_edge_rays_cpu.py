"""The companion-edge generator (tests/hero_edge_rays.py) on its own, no GPU, by the reference alone: it is deterministic, it gives
every camera its floor of guarded edges, it leaves out no more than its cap, and the edge column's record does not depend on where
the column stands nor on what the other columns trace."""
import numpy as np
import pytest

import hero_edge_rays as H
from hero_ref import same_words

MIN_GUARDED_EDGES = 1024       # usable guarded edges per camera, summed over the two lam_c
LEFT_OUT_CAP = 0.05            # of the edges that are neither at interface 0 nor of kind `other`, per camera and lam_c


@pytest.mark.parametrize("name", H.CAMERAS)
def test_companion_edges(oracle_lib, name):
    ce = H.edges(oracle_lib, name)
    print(H.tally_line(name, ce))
    n, per = len(ce["samples"]), ce["per_edge"]
    # deterministic: a second run of the generator, past the cache, gives equal arrays
    cached = dict(H._EDGES)
    H._EDGES.clear()
    again = H.edges(oracle_lib, name)
    H._EDGES.clear()
    H._EDGES.update(cached)
    assert again is not ce and H.edges(oracle_lib, name) is ce
    for key in ("samples", "hero", "lam_c", "states"):
        assert np.array_equal(ce[key].view(np.uint32), again[key].view(np.uint32)), key
    for key in ("edge", "offset", "guarded", "labels"):
        assert np.array_equal(ce[key], again[key]), key
    for key in ("margin", "band"):
        assert np.array_equal(ce[key], again[key], equal_nan=True), key
    assert ce["tally"] == again["tally"]
    # the floor: usable guarded edges, every one with all of its rows
    assert n % per == 0 and (np.bincount(ce["edge"])[np.unique(ce["edge"])] == per).all()
    guarded_edges = len(np.unique(ce["edge"][ce["guarded"]]))
    assert guarded_edges >= MIN_GUARDED_EDGES, (name, guarded_edges)
    assert sum(t["usable"] for t in ce["tally"].values()) * per == n
    # the cap on what is left out: a condition on the inputs, met by the reference alone
    for w, t in ce["tally"].items():
        candidates = t["found"] - t["at_interface_0"] - t["other"]
        assert candidates == t["usable"] + t["left_out"]
        assert t["left_out"] <= LEFT_OUT_CAP * candidates, (name, w, t)
    # every guarded row's f64 margin at the two ends of its edge is inside the band
    ends = ce["guarded"] & np.isin(ce["offset"], [0, 1])
    assert (ce["margin"][ends] < ce["band"][ends]).all()
    # the edge column at k = 8 (column 7, and column 3) is the record the k = 2 table gives column 1, word for word
    two = H.reference(oracle_lib, ce, 2, 1)[0]
    for col in (7, 3):
        eight = H.reference(oracle_lib, ce, 8, col)[0]
        assert same_words(eight[:, col], two[:, 1]).all(), (name, col)
        assert same_words(eight[:, 0], two[:, 0]).all(), (name, col)

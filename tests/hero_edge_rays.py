"""Companion edges of a Kolb camera (a plain helper module, imported by tests/test_hero_edge_rays_cpu.py and
tests/test_hero_edge_rays_gpu.py): hero rows whose COMPANION's one trace sits where the reference's f32 rounding decides a clip.

The FAST modes promise that every clip decision is a FAST one outside its guard band or a STRICT one (csrc/spectral.hip), hero tries
and companions alike.  tests/edge_rays.py places single-wavelength first tries on the edges; here the same rays become companions:

* an edge ray of edge_rays.edge_rays(..., ior=<the index table at lam_c>) is a sample whose first try flips between two adjacent f32
  lens samples at lam_c;
* run as a hero row (lam_h, lam_c) with a hero wavelength lam_h at which the oracle accepts the first try, the hero's accepted start
  is the sample's own first-try start, and the companion's one trace is the edge ray's first try at lam_c: its decision sits in the
  band.

An edge is USABLE under lam_h when, in hero_ref.hero_reference of the two-column rows (lam_h, lam_c), all of its 2 + 2 neighbours rows
have a hero accepted at try 0 with weight != 0 (flags & 0x3f == 0) and the companion's RAY_COMPANION_LOST bit differs between the
rows at offsets 0 and 1.  An edge takes the first lam_h of `heroes` under which it is usable.  Edges at interface 0 are geometry only
(the hit point there does not depend on the wavelength: the hero sits on them itself) and edges of kind `other` are jumps of the lens
sampler: neither is a companion edge.  A housing edge whose f64 margin at offset 0 or 1 is not below its interface's band is dropped
and counted as left out, like an edge no hero wavelength makes usable: there the f64 restatement cannot vouch that the row lies where
the guard must act (triplet-4's second interface from the front: the reference's own f32 rounding puts 2.6-2.9 % of its edges at
1.0-1.8 bands).

Everything is a pure function of its arguments; the results are cached and read-only."""
import numpy as np

from zoic_amd.workloads import ray_rng_states

import edge_rays as E
import hero_cases as hr
from differentials_ref import kolb_start
from fuzz_cameras import perturbed_prescription
from hero_ref import LOST, hero_reference
from spectral_ref import spectral_iors

F32 = np.float32
LAM_C = (400.0, 700.0)
HEROES = (486.1327, 830.0, 360.0)
# the seven cameras of the companion-edge tests: two shipped ones, the machine-made tessar of test_spectral_edge_rays and four lenses
# of the pinned corpus (the near-hemispherical rear element, the most and the fewest interfaces, the stop at trace index 0)
CAMERAS = ["C2", "C5", "abbe-lens", "rear-9", "fisheye-5", "triplet-4", "mori-6"]
ABBE_LENS = ("tessar_f2.8.dat", 21, 0.1, "keep")
ABBE_LENS_KW = dict(focalLength=5.0, fStop=2.8, focalDistance=120.0)
_SPECS = {}
_EDGES = {}


def spec(oracle_lib, name):
    """the hero_cases.Spec of camera `name`"""
    if name != "abbe-lens":
        return hr.spec(name)
    if name not in _SPECS:
        _SPECS[name] = hr.Spec(dict(oracle_lib.DEFAULTS, **ABBE_LENS_KW), lens=perturbed_prescription(*ABBE_LENS, abbe=True))
    return _SPECS[name]


def _frozen(a):
    a.setflags(write=False)
    return a


def companion_edges(oracle_lib, p, dispersion, lens_text=None, abbe=None, lam_c=LAM_C, heroes=HEROES, seed=13, neighbours=4):
    """The companion-edge rows of one camera (p: update() keyword arguments; dispersion: the camera's dispersion table; lens_text and
    abbe: its prescription and V-numbers where it is given them -- abbe is carried along for the caller that builds the camera).

    Returns a dict of read-only arrays over the n rows: samples (n, 4) f32; hero (n,), lam_c (n,) f32; states (n, 4) =
    ray_rng_states(n, seed=2); edge (the index of the row's edge, unique over both lam_c); offset (0 / 1: the two adjacent samples,
    < 0 and > 1: ulp neighbours beyond them); guarded (edge_rays.is_guarded); labels (str); margin, band (f64, housing edges) -- and
    tally: per lam_c a dict of edge counts, found = at_interface_0 + other + usable + left_out and left_out = no_hero + outside_band."""
    key = (lens_text, tuple(sorted(p.items())), None if abbe is None else np.asarray(abbe, F32).tobytes(), tuple(lam_c), tuple(heroes), seed,
           neighbours)
    if key in _EDGES:
        return _EDGES[key]
    per = 2 + 2 * neighbours
    at0, at1 = neighbours, neighbours + 1              # the rows of an edge at offsets 0 and 1
    housing = E.KINDS.index("housing")
    parts, tally, edges_before = [], {}, 0
    for w in lam_c:
        w = F32(w)
        er = E.edge_rays(oracle_lib, p, lens_text=lens_text, ior=spectral_iors(dispersion["ior_d"], dispersion["cauchy_b"], w), seed=seed,
                         stop_edges=0, nonstop_edges=0, min_rays=4096, lut_screens=0, max_batches=2, neighbours=neighbours)
        n_edges = len(er["pairs"])
        S = er["samples"].reshape(n_edges, per, 4)
        assert np.array_equal(er["offset"].reshape(n_edges, per)[:, at0:at1 + 1], np.tile([0, 1], (n_edges, 1)))
        first_iface = er["iface_e"] == 0
        other = er["kind_e"] == E.KINDS.index("other")
        candidate = ~first_iface & ~other
        hero = np.zeros(n_edges, F32)
        left = candidate.copy()
        for h in heroes:
            idx = np.nonzero(left)[0]
            if not len(idx):
                break
            s = np.ascontiguousarray(S[idx].reshape(-1, 4))
            lam = np.stack([np.full(len(s), h, F32), np.full(len(s), w, F32)], 1)
            words, _, det = hero_reference(oracle_lib, p, dispersion, s, lam, ray_rng_states(len(s), seed=2), lens_text=lens_text, details=True)
            first = (((det["flags"] & 0x3f) == 0) & (det["planes"][6] != 0)).reshape(-1, per)
            lost = ((words[:, 1, 7] & LOST) != 0).reshape(-1, per)
            ok = first.all(1) & (lost[:, at0] != lost[:, at1])
            hero[idx[ok]] = h
            left[idx[ok]] = False
        usable = candidate & ~left
        # a housing edge lies on the clip: the f64 margin of its two ends is inside the band the FAST modes guard
        m = er["margin"].reshape(n_edges, per)
        b = er["band"].reshape(n_edges, per)
        with np.errstate(invalid="ignore"):
            outside = (er["kind_e"] == housing) & ~((m[:, at0] < b[:, at0]) & (m[:, at1] < b[:, at1]))
        tally[float(w)] = dict(found=n_edges, at_interface_0=int(first_iface.sum()), other=int(other.sum()), usable=int((usable & ~outside).sum()),
                               left_out=int((candidate & ~(usable & ~outside)).sum()), no_hero=int((candidate & ~usable).sum()),
                               outside_band=int((usable & outside).sum()))
        usable &= ~outside
        rows = np.repeat(usable, per)
        parts.append(dict(samples=er["samples"][rows], hero=np.repeat(hero, per)[rows], lam_c=np.full(int(rows.sum()), w, F32),
                          edge=er["edge"][rows] + edges_before, offset=er["offset"][rows], guarded=E.is_guarded(er)[rows],
                          labels=E.labels(er)[rows], margin=er["margin"][rows], band=er["band"][rows]))
        edges_before += n_edges
    ce = {k: _frozen(np.ascontiguousarray(np.concatenate([q[k] for q in parts]))) for k in parts[0]}
    n = len(ce["samples"])
    ce["states"] = _frozen(ray_rng_states(n, seed=2))
    ce.update(tally=tally, per_edge=per, p=p, dispersion=dispersion, lens_text=lens_text, abbe=abbe, _refs={})
    # what makes the rows companion edges, on the rows as they are handed out: every hero accepted at try 0, the lost bit differing
    # across each edge, and the recorded start the sample's own first-try start bit for bit -- which is what carries edge_rays' kind,
    # iface, margin and band over to the companion
    words, _, det = reference(oracle_lib, ce, 2, 1)
    assert (((det["flags"] & 0x3f) == 0) & (det["planes"][6] != 0)).all()
    lost = ((words[:, 1, 7] & LOST) != 0).reshape(-1, per)
    assert (lost[:, at0] != lost[:, at1]).all()
    oc = E.oracle_camera(oracle_lib, p, lens_text)
    o0, d0 = kolb_start(oc, p, ce["samples"], np.zeros(n, np.int32), np.zeros((n, 4), np.uint32), oracle_lib)
    oc.close()
    assert np.array_equal(np.concatenate([o0, d0], 1).view(np.uint32), det["starts"].view(np.uint32)), "a hero's start is not its sample's first-try start"
    _EDGES[key] = ce
    return ce


def edges(oracle_lib, name):
    """companion_edges of camera `name` of CAMERAS"""
    sp = spec(oracle_lib, name)
    return companion_edges(oracle_lib, sp.params, sp.dispersion(), lens_text=sp.text, abbe=None if sp.lens is None else sp.lens.abbe)


def lambdas(ce, k, col, seed=5):
    """(n, k) float32: the hero in column 0, lam_c in column col, the other columns from hero_cases.palette"""
    assert 1 <= col < k
    lam = hr.palette(len(ce["samples"]), k, seed)
    lam[:, 0], lam[:, col] = ce["hero"], ce["lam_c"]
    return lam


def reference(oracle_lib, ce, k, col, seed=5):
    """hero_reference of the rows on lambdas(ce, k, col, seed), computed once: (words (n, k, 8), counters, details); read-only"""
    key = (k, col, seed)
    if key not in ce["_refs"]:
        words, counters, det = hero_reference(oracle_lib, ce["p"], ce["dispersion"], ce["samples"], lambdas(ce, k, col, seed), ce["states"],
                                              lens_text=ce["lens_text"], details=True)
        for a in (words, det["starts"], det["planes"], det["flags"]):
            a.setflags(write=False)
        ce["_refs"][key] = words, counters, det
    return ce["_refs"][key]


def tally_line(name, ce):
    """edges found / at interface 0 / of kind other / usable / left out, per lam_c, and the rows they make"""
    per_w = "; ".join("%g nm: found %d, at interface 0 %d, other %d, usable %d, left out %d (no hero %d, outside the band %d)" %
                      (w, t["found"], t["at_interface_0"], t["other"], t["usable"], t["left_out"], t["no_hero"], t["outside_band"])
                      for w, t in ce["tally"].items())
    labs, counts = np.unique(ce["labels"], return_counts=True)
    return "%s: %s | %d rows, %d guarded | rows per label %s" % (name, per_w, len(ce["samples"]), int(ce["guarded"].sum()),
                                                               {str(a): int(c) for a, c in zip(labs, counts)})

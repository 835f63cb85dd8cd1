"""Trace-back transmittance without a GPU (csrc/traceback_throughput.hpp): the C-ABI declares and exports the eight calls, the gfx950
kernels keep their budgets, and the host calls on tables-only cameras (zoic_trace_back_ray_transmittance, zoic_splat_point_transmittance
and their _spectral forms) leave the trace-back's Ps and flags untouched, agree with an f64 restatement (traceback_throughput_ref.py),
are reciprocal to the forward transmittance, and do what a lens designer expects.

Rays of the accuracy tests: the oracle's live d-line records of the 192 x 108 x 2 frame of traceback_cases -- C2 to C5 (a stride of at
most 8192, the V-numbers of backward_spectral_ref.DISPERSIVE) and the six ACCURACY lenses of the machine-made corpus (the leading live
records of machine_lens_corpus.ray_set, ~2 900) -- taken back at the d-line, 400, 486.1327, 656.2725 and 700 nm, bare and with
transmittance_ref.films_where_media_differ's 1.38 film at 550 nm.  Edge rays (TraceBack.edge: 1e-2 at the stop, 1e-4 elsewhere; at
most EDGE_CAP of a lens's rays at any wavelength, asserted on the f64 trace alone) are left out; off the edge set the decisions are
equal.  Compared rays per lens: the sum over the five wavelengths (a corpus lens has fewer than 4096 live records in its ray set).
Measured on the library's host build (hipcc's clang, x86-64), largest |T_host - T_f64| over the five wavelengths:

    lens        rays   compared   edge share (max)   bare        film        median T (d-line) bare / film   E_rec bare / film
    C2          6731    33 496      0.61 %           2.58e-7     2.85e-7     0.687 / 0.940                   2.0e-9 / 3.2e-9
    C3          6908    34 514      0.01 %           2.25e-7     3.18e-7     0.588 / 0.895                   2.9e-8 / 4.1e-8
    C4          6912    31 937      1.07 %           2.17e-7     4.71e-7     0.532 / 0.906                   5.3e-8 / 7.3e-8
    C5          4361    21 749      0.37 %           2.14e-7     3.62e-7     0.660 / 0.894                   2.6e-9 / 3.9e-9
    triplet-4   2823    14 110      0.04 %           1.55e-7     1.84e-7     0.764 / 0.982                   1.5e-9 / 2.6e-9
    fisheye-5   2962    14 340      1.22 %           2.23e-7     4.96e-7     0.530 / 0.908                   3.0e-9 / 6.8e-9
    mori-6      2962    14 729      0.10 %           1.74e-7     5.70e-7     0.472 / 0.962                   2.4e-9 / 1.3e-8
    double-3    2963    14 715      1.18 %           2.24e-7     2.85e-7     0.595 / 0.861                   1.3e-8 / 1.9e-8
    tessar-5    2835    14 143      0.21 %           2.51e-7     2.68e-7     0.679 / 0.871                   4.6e-9 / 6.6e-9
    petzval-2   2736    13 553      0.62 %           2.07e-7     2.57e-7     0.743 / 0.912                   2.2e-9 / 3.1e-9

No lens stands apart: one bound.  MEASURED = 5.695e-7 (mori-6 with the film) and BOUND = 4 x MEASURED = 2.278e-6, the margin for other
compilers' host builds (the convention of tests/test_transmittance_cpu.py).

Reciprocity.  E_rec = |T_back_f64(record) - T_fwd_f64(start)|, reference against reference: non-zero only because the record's origin
and dir are f32.  A path is reciprocal to itself, so it is taken where the record is the path: the d-line runs (the records are d-line
records; taken back at 400 nm they follow another path than their starts).  Largest E_rec: 7.33e-8 (C4 with the film); the host's
|T_back - T_fwd_f64| reaches 3.1e-7 and is held to BOUND + max E_rec of its own run."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from zoic_amd import ZoicCamera, _capi
from zoic_amd.camera import LENS_DIR, ZoicError
from zoic_amd.workloads import camera_params, ray_rng_states

import backward_spectral_ref as bs
import edge_rays as E
import machine_lens_corpus as mc
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr
import transmittance_ref as tref
from device_cases import bits_f32 as _bits
from library_facts import header_text, kernel_resources
from machine_lens_corpus import EDGE_CAP

NEW = ("zoic_trace_back_transmittance_device", "zoic_trace_back_transmittance_spectral_device", "zoic_trace_back_ray_transmittance",
       "zoic_trace_back_ray_transmittance_spectral", "zoic_splat_transmittance_device", "zoic_splat_transmittance_spectral_device",
       "zoic_splat_point_transmittance", "zoic_splat_point_transmittance_spectral")
F32 = np.float32
MEASURED, BOUND, E_REC = tr.MEASURED, tr.BOUND, tr.E_REC      # (the device tests read them too)
INVALID = _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
NO_DEVICE = _capi.STATUS_NAMES.index("ZOIC_ERR_NO_DEVICE")
NOT_UPDATED = _capi.STATUS_NAMES.index("ZOIC_ERR_NOT_UPDATED")
ODD_WAVELENGTHS = (587.5618, 359.0, 831.0, np.nan, 400.0, 700.0, 360.0, 830.0)


# ---- 1. symbols and budgets ------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_calls():
    text = header_text()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SYMBOLS and hasattr(raw, name) and hasattr(_capi.load(), name), name
    assert _capi.load().zoic_abi_version() == 5 and _capi.ABI_VERSION == 5


def test_kernel_budgets():
    res = kernel_resources()
    ray = {k: v for k, v in res.items() if "tb_throughput_kernel" in k}
    aim = {k: v for k, v in res.items() if "aim_throughput_kernel" in k}
    assert len(ray) == 3 and len(aim) == 3, (sorted(ray), sorted(aim))   # an instance per lens model each
    for k, v in dict(ray, **aim).items():
        print(k, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0 and v["kernarg"] <= 4096, (k, v)
        for word in ("transmittance", "splat", "ghost", "pupil_bounds", "differentials_kernel", "spectral_diff", "trace_back_jacobian",
                     "trace_back_kernel", "hero"):
            assert word not in k, (k, word)     # the substrings the other budget tests count kernels by
    splat = [v for k, v in res.items() if k.startswith("splat_kernel<1>")]
    assert len(splat) == 1
    for k, v in ray.items():
        assert v["vgpr"] <= 96, (k, v)
    for k, v in aim.items():
        if "<1>" in k:      # RAYTRACED: without the tangents, no more than the fused splat kernel
            assert v["vgpr"] <= min(79, splat[0]["vgpr"]), (k, v, splat[0])


# ---- 2. the trace is untouched -----------------------------------------------------------------------------------------------------------
def _camera(p):
    return tc.update(ZoicCamera(device=-1), p)


def _same_trace(cam, o, d):
    """Ps and flags of the transmittance calls against the trace-back calls', bit for bit, at the d-line, at 587.5618f and at a mix
    of wavelengths; the rules T obeys.  Returns (flags, T) of the mixed run."""
    ps0, fl0 = tc.lib_trace(cam, o, d)
    ps, fl, T = tr.lib_throughput(cam, o, d)
    assert np.array_equal(fl, fl0) and np.array_equal(_bits(ps), _bits(ps0))
    psd, fld, Td = tr.lib_throughput(cam, o, d, tr.LAMBDA_D32)
    assert np.array_equal(fld, fl) and np.array_equal(_bits(psd), _bits(ps)) and np.array_equal(_bits(Td), _bits(T))
    lam = np.array([ODD_WAVELENGTHS[i % len(ODD_WAVELENGTHS)] for i in range(len(o))], F32)
    ps1, fl1 = tc.lib_trace(cam, o, d, lam)
    psm, flm, Tm = tr.lib_throughput(cam, o, d, lam)
    assert np.array_equal(flm, fl1) and np.array_equal(_bits(psm), _bits(ps1))
    assert (tc.reason(flm[~bs.valid(lam)]) == bs.TB_WAVELENGTH).all()
    for f, t in ((fl, T), (flm, Tm)):
        traced = (f & 1) == 1
        assert np.array_equal(t > 0, traced)
        assert (_bits(t[~traced]) == 0).all()              # +0.0, the sign bit clear
        assert (t[traced] <= 1.0).all()
    return flm, Tm


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_screen_sample_and_flags_are_the_trace_backs(oracle_lib, name):
    p = tc.params_of(name)
    cam = _camera(p)
    kolb = name in tc.KOLB
    if kolb:
        bs.set_dispersion(cam, name)
        if name in ("C3", "C5", "triplet"):
            tr.coat(cam, tref.films_where_media_differ(cam.dispersion()))
    s, o, d, w = tc.oracle_records(oracle_lib, p)
    live = np.flatnonzero(w > 0)
    pick = mc.strided(live, 2048)
    fo, fd = bs.trace_back_rays(tc, cam.info(), (o[live], d[live], w[live]), kolb, per_family=256)
    keep = np.ones(len(fo), bool)
    keep[:len(live)] = False                         # (its first set is every live record: a stride of them is enough here)
    O, D = np.concatenate([o[pick].astype(F32), fo[keep]]), np.concatenate([d[pick].astype(F32), fd[keep]])
    fl, T = _same_trace(cam, O, D)
    seen = set(tc.reason(fl[(fl & 1) == 0]).tolist())
    print(name, len(O), "rays; reasons", sorted(seen), "; traced", int((fl & 1).sum()))
    assert (fl & 1).sum() >= 512 and len(seen) >= (5 if kolb else 3), seen
    if not kolb:      # THINLENS: no interface
        assert (T[(fl & 1) == 1] == 1.0).all()
    else:
        assert (T[(fl & 1) == 1] < 1.0).all()
    cam.close()


def test_edge_rays_and_refusing_cameras(oracle_lib):
    """the forward records of samples placed ON the clip edges (edge_rays.py), and the cameras that refuse every ray"""
    p = camera_params("C5")
    er = E.edge_rays(oracle_lib, p, seed=4, screens=128, lut_screens=32)
    oc = E.oracle_camera(oracle_lib, p)
    smp = mc.strided(er["samples"], 4096)
    r = oc.create_rays(smp, rng_states=ray_rng_states(len(smp), seed=9))
    oc.close()
    live = r["weight"] > 0
    assert live.sum() >= 1024
    cam = _camera(p)
    _same_trace(cam, r["origin"].T[live].astype(F32), r["dir"].T[live].astype(F32))
    cam.close()
    ray = ((0.05, 0.02, -3.0), (0.01, -0.02, -1.0))
    o, d = tc.non_finite_rays()
    o, d = np.concatenate([o, [ray[0]]]).astype(F32), np.concatenate([d, [ray[1]]]).astype(F32)
    for over in (dict(camera_params("C3"), lensModel=_capi.LENS_NONE), dict(camera_params("C3"), focalLength=-10.0),
                 dict(camera_params("C1"), useDof=False)):
        cam = _camera(over)
        fl, T = _same_trace(cam, o, d)
        assert ((fl & 1) == 0).all() and (_bits(T) == 0).all()
        sx, sy, f, t = cam.trace_back_ray_transmittance(*ray)
        assert (sx, sy, f) == cam.trace_back_ray(*ray) and t == 0.0 and np.signbit(F32(t)) == False   # noqa: E712
        cam.close()


# ---- 3. accuracy against f64 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(oracle_lib, name, coated):
    """the host calls on lens `name` at the five wavelengths, against the restatement: dict of per-wavelength (ref, edge, T64, flags, T)
    and the run's figures.  Shared by the tests below; read only."""
    L = tr.lens(oracle_lib, name)
    tr.coat(L.cam, L.films if coated else None)
    out = {}
    for lam in tr.WAVELENGTHS:
        ref, edge, T64 = L.reference(lam, coated)
        ps, fl, T = tr.lib_throughput(L.cam, L.o, L.d, lam)
        out[lam] = ref, edge, T64, fl, T
    return out


@pytest.mark.parametrize("name", tr.LENSES)
def test_reference_only_conditions(oracle_lib, name):
    """asserted on the f64 trace alone, before the library is looked at: the edge share at every wavelength"""
    L = tr.lens(oracle_lib, name)
    for lam in tr.WAVELENGTHS:
        ref, edge, _ = L.reference(lam, False)
        print(name, lam, "edge share %.4f, non-edge traced %d of %d" % (edge.mean(), (ref["traced"] & ~edge).sum(), len(edge)))
        assert edge.mean() <= EDGE_CAP, (name, lam, edge.mean())


@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", tr.LENSES)
def test_host_build_against_f64(oracle_lib, name, coated):
    worst, compared = 0.0, 0
    for lam, (ref, edge, T64, fl, T) in _run(oracle_lib, name, coated).items():
        ok = (fl & 1) == 1
        assert np.array_equal(ok[~edge], ref["traced"][~edge]), (name, lam)      # equal decisions off the edge set
        both = ~edge & ok
        err = np.abs(T.astype(np.float64) - T64)[both]
        assert (T[both] > 0).all() and (T[both] < 1).all()
        worst, compared = max(worst, float(err.max())), compared + int(both.sum())
    print("%-10s %s: rays %d, compared %d, largest |T_host - T_f64| %.3e" % (name, "film" if coated else "bare", len(edge), compared, worst))
    assert compared >= 4096, compared
    assert worst <= BOUND, (name, coated, worst)


def test_measured_bound_is_the_measured_one(oracle_lib):
    """MEASURED is what these runs give on the build it was taken from, not a round figure: the largest error of the lens that set it,
    and of the largest bare run, lie within [MEASURED / 4, 4 MEASURED] on any host build"""
    worst = 0.0
    for name, coated in (("mori-6", True), ("C2", False)):
        for lam, (ref, edge, T64, fl, T) in _run(oracle_lib, name, coated).items():
            both = ~edge & ((fl & 1) == 1)
            worst = max(worst, float(np.abs(T.astype(np.float64) - T64)[both].max()))
    assert MEASURED / 4 <= worst <= BOUND, worst


# ---- 4. reciprocity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coated", [False, True], ids=["bare", "film"])
@pytest.mark.parametrize("name", tr.LENSES)
def test_reciprocity(oracle_lib, name, coated):
    """the backward T of a forward record equals the forward T of its start: |T_host_back - T_fwd_f64| <= BOUND + max E_rec, E_rec the
    same difference between the two f64 restatements (printed; the module's docstring has the table)"""
    L = tr.lens(oracle_lib, name)
    ref, edge, T64, fl, T = _run(oracle_lib, name, coated)[None]
    Tf, passes = tr.forward_transmittance(L.info, L.disp, L.o0, L.d0, tr.LAMBDA_D32, L.films if coated else None)
    both = ~edge & ((fl & 1) == 1)
    assert passes[both].all()
    e_rec = float(np.abs(T64 - Tf)[both].max())
    got = float(np.abs(T.astype(np.float64) - Tf)[both].max())
    print("%-10s %s: E_rec max %.3g, |T_host_back - T_fwd_f64| max %.3g" % (name, "film" if coated else "bare", e_rec, got))
    assert e_rec <= 4 * E_REC         # the yardstick itself is small: the two restatements describe one path
    assert got <= BOUND + e_rec, (got, e_rec)


# ---- 5. physics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", tref.LENSES)
def test_axial_ray_meets_the_closed_form(lens):
    p = dict(camera_params("C2"), lensDataPath=os.path.join(LENS_DIR, lens))
    cam = _camera(p)
    disp = cam.dispersion()
    sx, sy, f, t = cam.trace_back_ray_transmittance((0.0, 0.0, -50.0), (0.0, 0.0, -1.0))
    want = tref.on_axis_closed_form(disp["ior_d"])
    print(lens, t, want)
    assert f & 1 and abs(t - want) <= BOUND, (lens, t, want)
    # the ideal film: nc = sqrt(n1 n2), a quarter wave thick at the ray's wavelength, met along the axis: nothing is reflected
    n1 = disp["ior_d"].astype(np.float64)
    n2 = np.append(n1[1:], 1.0)
    nc = np.where(n1 != n2, np.sqrt(n1 * n2), 0.0).astype(F32)
    tr.coat(cam, (nc, np.full(len(nc), tr.LAMBDA_D32, F32)))
    t_ideal = cam.trace_back_ray_transmittance((0.0, 0.0, -50.0), (0.0, 0.0, -1.0))[3]
    assert 0.0 < t_ideal <= 1.0 and 1.0 - t_ideal <= BOUND, (lens, t_ideal)
    cam.close()


@pytest.mark.parametrize("name", tr.LENSES)
def test_the_film_lets_more_light_through(oracle_lib, name):
    med = []
    for coated in (False, True):
        ref, edge, T64, fl, T = _run(oracle_lib, name, coated)[None]
        med.append(float(np.median(T[~edge & ((fl & 1) == 1)])))
    print(name, "median T bare %.4f, film %.4f" % tuple(med))
    assert med[1] > med[0]


def test_setters_show_in_the_next_call_without_an_update():
    p = tc.params_of("C2")
    cam = _camera(p)
    ray = ((0.3, -0.2, -40.0), (0.004, -0.003, -1.0))
    bare = cam.trace_back_ray_transmittance(*ray)
    assert bare[2] & 1
    films = tref.films_where_media_differ(cam.dispersion())
    tr.coat(cam, films)
    film = cam.trace_back_ray_transmittance(*ray)
    assert film[:3] == bare[:3] and film[3] > bare[3]
    tr.coat(cam, None)
    assert cam.trace_back_ray_transmittance(*ray) == bare
    blue = cam.trace_back_ray_transmittance(*ray, wavelength=420.0)
    cam.set_abbe_numbers(np.full(cam.info()["lensCount"], 25.0, F32))
    assert cam.trace_back_ray_transmittance(*ray) == bare                       # the d-line does not see a V-number
    blue25 = cam.trace_back_ray_transmittance(*ray, wavelength=420.0)
    assert blue25[2] & 1 and blue25 != blue and blue25[:3] == cam.trace_back_ray(*ray, wavelength=420.0)
    cam.set_abbe_numbers(None)
    assert cam.trace_back_ray_transmittance(*ray, wavelength=420.0) == blue
    cam.close()


# ---- 6. the splat side ---------------------------------------------------------------------------------------------------------------------
AIMS = (1, 5, 64)


def _u(n, m, seed=21):
    u = np.random.default_rng(seed + m).random((n, m, 2)).astype(F32)
    u[0, 0] = 0.0
    return u


@pytest.mark.parametrize("spectral", [False, True], ids=["d-line", "spectral"])
@pytest.mark.parametrize("name", sorted(pc.CAMERAS))
def test_splat_side_equals_the_ray_side(name, spectral):
    """zoic_splat_point_transmittance against zoic_trace_back_ray_transmittance on the rays rebuilt from zoic_splat_point's recorded
    aims (origin P, dir P - A in numpy float32), bit for bit; T > 0 exactly where the splat record is traced"""
    p = pc.params_of(name)
    cam = _camera(p)
    cfg = pc.CAMERAS[name][0]
    if cfg in tc.KOLB:
        bs.set_dispersion(cam, cfg)
        tr.coat(cam, tref.films_where_media_differ(cam.dispersion()))
    pts = pc.points(p)
    lam = pc.wavelengths(len(pts)) if spectral else [None] * len(pts)
    z = F32(cam.pupil_square()[0])
    traced = boxes = 0
    for m in AIMS:
        u = _u(len(pts), m)
        for i, P in enumerate(pts):
            b = cam.pupil_bounds_point(P, 16)               # the d-line box: an invalid wavelength reaches the trace
            rec = cam.splat_point(P, b, u[i], lam[i])
            T = cam.splat_point_transmittance(P, b, u[i], lam[i])
            assert T.dtype == F32 and T.shape == (m,)
            none = rec["flags"] == _capi.SPLAT_NO_BOX
            assert np.array_equal(T > 0, (rec["flags"] & 1) == 1) and (_bits(T[~(T > 0)]) == 0).all(), (name, m, i)
            assert (T <= 1.0).all()
            go = ~none
            with np.errstate(invalid="ignore"):
                A = np.stack([rec["ax"][go], rec["ay"][go], np.full(go.sum(), z, F32)], 1).astype(F32)
                o = np.repeat(P[None, :], go.sum(), 0).astype(F32)
                d = (o - A).astype(F32)
            ps, fl, want = tr.lib_throughput(cam, o, d, None if lam[i] is None else lam[i])
            assert np.array_equal(fl, rec["flags"][go]) and np.array_equal(_bits(want), _bits(T[go])), (name, m, i)
            traced += int((T > 0).sum())
            boxes += int(none.sum())
            if spectral and lam[i] == F32(pc.BAD_LAMBDA):
                assert (_bits(T) == 0).all()
            if m == 5:      # a NaN u: a NaN aim, refused by the trace
                bad = u[i].copy()
                bad[2, 0] = np.nan
                Tn = cam.splat_point_transmittance(P, b, bad, lam[i])
                assert _bits(Tn[2:3])[0] == 0 and np.array_equal(_bits(np.delete(Tn, 2)), _bits(np.delete(T, 2)))
    print(name, "traced", traced, "empty boxes", boxes)
    assert traced >= (20 if name != "C5" else 1) and boxes >= AIMS[0] + AIMS[1] + AIMS[2]   # the point behind the lens, the NaN point
    cam.close()


def test_splat_no_box_and_d_line_pairing():
    """an empty box gives +0.0 whatever it holds; the d-line call is the spectral call at 587.5618f"""
    p = pc.params_of("C3")
    cam = _camera(p)
    P = pc.points(p)[3]
    b = cam.pupil_bounds_point(P, 16)
    u = _u(1, 5)[0]
    T = cam.splat_point_transmittance(P, b, u)
    assert (T > 0).any()
    assert np.array_equal(_bits(T), _bits(cam.splat_point_transmittance(P, b, u, 587.5618)))
    for change in (dict(count=0), dict(flags=b["flags"] & ~1)):
        assert (_bits(cam.splat_point_transmittance(P, dict(b, **change), u)) == 0).all()
    cam.close()


# ---- the interface on a tables-only camera ---------------------------------------------------------------------------------------------------
def test_errors_on_a_tables_only_camera():
    lib = _capi.load()
    o, d = _capi.Vec3(0.05, 0.02, -3.0), _capi.Vec3(0.0, 0.0, -1.0)
    ps = (ctypes.c_float * 2)(7.0, 7.0)
    f = ctypes.c_uint32(77)
    t = ctypes.c_float(7.0)
    ray, rays = lib.zoic_trace_back_ray_transmittance, lib.zoic_trace_back_ray_transmittance_spectral
    R = ctypes.byref
    assert ray(None, R(o), R(d), ps, R(f), R(t)) == INVALID
    fresh = ZoicCamera(device=-1)
    assert ray(fresh._h, R(o), R(d), ps, R(f), R(t)) == NOT_UPDATED
    with pytest.raises(ZoicError):
        fresh.trace_back_ray_transmittance((0.05, 0.02, -3.0), (0.0, 0.0, -1.0))
    fresh.close()
    p = tc.params_of("C2")
    cam = _camera(p)
    h = cam._h
    assert ray(h, None, R(d), ps, R(f), R(t)) == INVALID and ray(h, R(o), None, ps, R(f), R(t)) == INVALID
    assert ray(h, R(o), R(d), ps, R(f), None) == INVALID and rays(h, R(o), R(d), 500.0, ps, R(f), None) == INVALID
    assert (ps[0], ps[1], f.value, t.value) == (7.0, 7.0, 77, 7.0)              # an argument error writes nothing
    assert ray(h, R(o), R(d), None, None, R(t)) == 0 and 0.0 < t.value < 1.0     # Ps and flags may be NULL
    assert rays(h, R(o), R(d), 500.0, None, None, R(t)) == 0 and 0.0 < t.value < 1.0
    # the device calls: no device comes before everything else on a tables-only camera, as for the other batch calls
    assert lib.zoic_trace_back_transmittance_device(None, 4, None, None, None, None, None) == INVALID
    assert lib.zoic_trace_back_transmittance_device(h, 4, None, None, None, None, None) == NO_DEVICE
    assert lib.zoic_trace_back_transmittance_spectral_device(h, 4, None, None, None, None, None, None) == NO_DEVICE
    assert lib.zoic_splat_transmittance_device(h, 4, None, None, 0, None, None, None) == INVALID        # m = 0 with n > 0
    assert lib.zoic_splat_transmittance_spectral_device(h, 4, None, None, None, 0, None, None, None) == INVALID
    assert lib.zoic_splat_transmittance_device(h, 4, None, None, 1, None, None, None) == NO_DEVICE
    assert lib.zoic_splat_transmittance_spectral_device(h, 4, None, None, None, 1, None, None, None) == NO_DEVICE
    for call, args in ((cam.trace_back_transmittance, (np.zeros((4, 8), F32),)),
                       (cam.splat_transmittance, (np.zeros((4, 3), F32), np.zeros((4, 12), F32), np.zeros((4, 2, 2), F32)))):
        with pytest.raises(ZoicError) as e:
            call(*args)
        assert e.value.status_name == "ZOIC_ERR_NO_DEVICE"
    # the host splat calls: a sentinel-filled output stays as it was on every argument error
    P = pc.points(p)[3]
    b = _capi.PupilBounds.from_buffer_copy(np.zeros(1, _capi.PUPIL_BOUNDS_DTYPE).tobytes())
    po = _capi.Vec3(*[float(v) for v in P])
    u = np.full((4, 2), 0.5, F32)
    T = np.full(4, 7.0, F32)
    up, tp = u.ctypes.data_as(ctypes.c_void_p), T.ctypes.data_as(ctypes.c_void_p)
    one, two = lib.zoic_splat_point_transmittance, lib.zoic_splat_point_transmittance_spectral
    assert one(h, R(po), R(b), 0, up, tp) == INVALID and two(h, R(po), R(b), 500.0, 0, up, tp) == INVALID
    assert one(h, None, R(b), 4, up, tp) == INVALID and one(h, R(po), None, 4, up, tp) == INVALID
    assert one(h, R(po), R(b), 4, None, tp) == INVALID and one(h, R(po), R(b), 4, up, None) == INVALID
    assert one(h, R(po), R(b), 4, ctypes.c_void_p(u.ctypes.data + 2), tp) == INVALID                      # a misaligned u
    assert one(h, R(po), R(b), 4, up, ctypes.c_void_p(T.ctypes.data + 2)) == INVALID                      # a misaligned T
    assert one(None, R(po), R(b), 4, up, tp) == INVALID
    assert (T == 7.0).all()
    assert one(h, R(po), R(b), 4, up, tp) == 0 and (_bits(T) == 0).all()                                  # the empty box
    cam.close()

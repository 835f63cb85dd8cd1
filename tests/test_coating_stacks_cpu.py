"""Multilayer coatings without a GPU: the arithmetic of csrc/coating_stack.hpp (compiled for the host, coating_stack_drivers.py)
against the f64 complex transfer-matrix restatement (coating_stack_ref.py) -- the two phase polynomials, the interface function on a
grid, the equivalence with the single film, the physics a coating designer expects, the four paths that price an interface
(forward transmittance, ghosts, trace-back and splat transmittance) on C2 - C5 -- and the budget of the gfx950 kernels.

Every figure below was measured on the build the bounds were taken from (clang++ 22, x86-64); what is asserted is 4 x the measured
figure, the project's margin for other compilers' host builds (test_transmittance_cpu.py)."""
import numpy as np
import pytest

from zoic_amd import ZoicCamera, _capi

import backward_spectral_ref as bs
import coating_stack_drivers as cd
import coating_stack_ref as cr
import ghost_ref as gref
import host_drivers
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr
import transmittance_ref as tref
from coating_stack_ref import NAMED, Q, QHQ, R8, THICK, f32_pairs
from device_cases import bits_f32 as _bits
from differentials_spectral_ref import lens_rays as _rays, ray_wavelengths as _wavelengths, tables
from host_drivers import split_ghost as split
from library_facts import kernel_resources
from transmittance_ref import housings

F32 = np.float32
CFGS = ["C2", "C3", "C4", "C5"]
LAMBDA_D32 = F32(587.5618)

# film_sinpi / film_cospi: largest error against f64 sin(pi x) / cos(pi x) on 10^5 points of [0, 22.3], and what is asserted -- the
# measured figure with the margin test_transmittance_cpu.py gives COSPI_BOUND (2e-7 for 1.014e-7: a factor 1.97)
SINPI_MEASURED, COSPI_MEASURED = 1.735e-7, 1.013e-7
SINPI_BOUND, COSPI_BOUND = 3.5e-7, 2e-7
# the interface function on the grid of test_interface_against_f64: largest |T_f32 - T_f64| per stack
MEASURED = dict(Q=1.622e-7, QHQ=1.363e-6, R8=3.080e-6, THICK=6.390e-6)
BOUND = {k: 4 * v for k, v in MEASURED.items()}
# the paths: largest |host build - f64 restatement| per lens, the larger of the QHQ run and the R8 run (test_paths_against_f64 prints both)
PATH_MEASURED = dict(
    forward=dict(C2=3.537e-6, C3=3.027e-6, C4=3.132e-6, C5=2.884e-6),      # QHQ alone: 3.9e-7, 3.9e-7, 4.5e-7, 3.8e-7
    back=dict(C2=1.698e-6, C3=8.991e-7, C4=1.428e-6, C5=1.029e-6),         # QHQ alone: 2.6e-7, 3.3e-7, 3.1e-7, 2.9e-7
    ghost=dict(C2=1.964e-7, C3=9.627e-7, C4=3.553e-7, C5=1.198e-7),        # weights; QHQ alone: 1.9e-8, 1.0e-8, 1.4e-8, 8.2e-9
)
E_REC = 1.099e-7     # largest |T_back_f64(record) - T_fwd_f64(start)| under the stacks, reference against reference (test_reciprocity)
FILM_PATH_BOUND = 4 * 3.354e-7   # the single film's path: BOUND of test_transmittance_cpu.py (4 x its MEASURED)
MARGIN = 1e-4   # test_ghost_cpu.py's: ghosts whose f64 decisions lie closer than this are left out


@pytest.fixture(scope="module")
def driver():
    return cd.driver()


# ---- 2. the phase polynomials -----------------------------------------------------------------------------------------------------
def test_phase_polynomials(driver):
    """x = 2 n d cc / lambda reaches 2 x 4 x 1000 / 360 = 22.3 under the setter's limits"""
    x = np.linspace(0.0, 22.3, 100000).astype(F32)
    s, c, s2, c2 = cd.sincos(driver, x)
    x64 = x.astype(np.float64)
    es, ec = np.abs(s - np.sin(np.pi * x64)), np.abs(c - np.cos(np.pi * x64))
    print("film_sinpi: largest error %.4e at x = %.6f; film_cospi: %.4e at x = %.6f" % (es.max(), x[es.argmax()], ec.max(), x[ec.argmax()]))
    assert es.max() <= SINPI_BOUND and ec.max() <= COSPI_BOUND
    assert SINPI_MEASURED / 4 <= es.max() and COSPI_MEASURED / 4 <= ec.max()
    # the layer loop's fused form has the two functions' bits
    assert np.array_equal(_bits(s), _bits(s2)) and np.array_equal(_bits(c), _bits(c2))
    # the reduction is exact: at the integers and half-integers up to 22 the polynomials see 0 and +-1/2
    k = np.arange(0, 23, dtype=F32)
    s, c = cd.sincos(driver, k)[:2]
    assert not s.any() and np.array_equal(c, np.where(k % 2 == 0, 1.0, -1.0).astype(F32))
    s, c = cd.sincos(driver, k + F32(0.5))[:2]
    assert np.abs(np.abs(s) - 1.0).max() <= SINPI_BOUND and np.abs(c).max() <= COSPI_BOUND


# ---- 3. the interface function ----------------------------------------------------------------------------------------------------
MEDIA = [(1.0, 1.52), (1.0, 1.8), (1.52, 1.0), (1.8, 1.0), (1.65, 1.5), (1.0, 1.0003)]
DENORMAL = float(np.nextafter(F32(0), F32(1)))


def _grid(n1, n2):
    """(ci, ct, lambda) float32 of the grid for the media n1 -> n2: ci = 0, the smallest denormal, 1, 40 values between, and -- where
    n1 > n2 -- four either side of the critical angle's cosine within a few ulps of ct = 0; six wavelengths over [360, 830]"""
    n1, n2 = F32(n1), F32(n2)
    ci = np.concatenate([[0.0, DENORMAL, 1.0], np.linspace(0.02, 0.999, 40)]).astype(F32)
    if n1 > n2:
        crit = F32(np.sqrt(1.0 - (float(n2) / float(n1)) ** 2))
        near = [crit]
        for _ in range(4):
            near = [np.nextafter(near[0], F32(0))] + near + [np.nextafter(near[-1], F32(2))]
        ci = np.concatenate([ci, np.array(near, F32)])
    lam = np.array([360.0, 450.0, 550.0, 587.5618, 650.0, 830.0], F32)
    CI, LA = (a.ravel() for a in np.meshgrid(ci, lam, indexing="ij"))
    eta = F32(n1 / n2)
    k2 = F32(1) - (eta * eta) * (F32(1) - CI * CI)
    ok = k2 >= 0                        # the trace hands over no totally reflected ray
    return CI[ok], np.sqrt(k2[ok]).astype(F32), LA[ok]


@pytest.mark.parametrize("name", list(NAMED))
def test_interface_against_f64(name, driver):
    """Q, QHQ, R8 and THICK met forwards and backwards on the grid: finite and in [0, 1] everywhere, and within BOUND of the f64
    restatement.  Measured: Q 1.622e-7, QHQ 1.363e-6, R8 3.080e-6, THICK 6.390e-6 (the phase x reaches 22: its f32 rounding)."""
    stack = f32_pairs(NAMED[name])
    worst, points, near_critical = 0.0, 0, 0
    for n1, n2 in MEDIA:
        ci, ct, lam = _grid(n1, n2)
        near_critical += int(((ct < 1e-3) & (ci > 0)).sum())
        for forward in (True, False):
            got = cd.run_interface(driver, n1, n2, ci, ct, lam, stack, forward)
            assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), (name, n1, n2, forward)
            ref = cr.stack_transmittance(F32(n1), F32(n2), ci, ct, stack if forward else stack[::-1], lam)
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
            points += len(got)
            zero = ci == 0                                               # grazing incidence: everything is reflected, T = +0.0
            assert (zero.any() or n1 > n2) and (_bits(got[zero]) == 0).all()
    print(name, "points", points, "near the critical angle", near_critical, "largest |T_f32 - T_f64| %.4e" % worst)
    assert near_critical >= 12 and points >= 2000
    assert MEASURED[name] / 4 <= worst <= BOUND[name], (name, worst)


def _crit():
    """(n1, ci, index): eight equal layers of `index` put cc at its smallest non-zero value, 2^-12, for (n1, ci): the largest
    (n1 / index)^2 (1 - ci^2) below 1 in the header's f32 operations"""
    n1, ci = F32(1.8), F32(0.5)
    sin2 = F32(1) - ci * ci
    nj = F32(float(n1) * np.sqrt(float(sin2)))
    best = None
    for _ in range(64):
        nj = np.nextafter(nj, F32(0))
    for _ in range(128):
        q = n1 / nj
        s2 = (q * q) * sin2
        if s2 < 1 and (best is None or s2 > best[1]):
            best = (nj, s2)
        nj = np.nextafter(nj, F32(4))
    assert best is not None and best[1] == np.nextafter(F32(1), F32(0)), best
    return n1, ci, best[0]


def test_crit_and_the_evanescent_rule(driver):
    """CRIT: eight near-critical layers, 1000 nm each, stay finite and in [0, 1] (the matrix is rescaled by powers of two), at the
    chosen cosine, a few ulps around it and on the whole grid; and a layer without a wave gives the bare interface's bits"""
    n1, ci0, index = _crit()
    for thick in (1000.0, 137.0, 1e-3):
        stack = [(float(index), thick)] * 8
        near = [ci0]
        for _ in range(3):
            near = [np.nextafter(near[0], F32(0))] + near + [np.nextafter(near[-1], F32(1))]
        ci = np.array(near, F32)
        for n2 in (1.6, 1.79, 2.0):                     # (n1 sin i = 1.559: a rarer second medium reflects the ray totally)
            eta = n1 / F32(n2)
            k2 = F32(1) - (eta * eta) * (F32(1) - ci * ci)
            ok = k2 >= 0
            ct = np.sqrt(np.where(ok, k2, 0)).astype(F32)
            for lam in (360.0, 550.0, 830.0):
                for forward in (True, False):
                    got = cd.run_interface(driver, n1, n2, ci[ok], ct[ok], lam, stack, forward)
                    bare = cd.run_interface(driver, n1, n2, ci[ok], ct[ok], lam, [])
                    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), (thick, n2, lam, got)
                    q = n1 / index
                    evan = ~((q * q) * (F32(1) - ci[ok] * ci[ok]) < 1)
                    assert evan.any() and (~evan).any()
                    assert np.array_equal(_bits(got[evan]), _bits(bare[evan]))         # the rule, with >= : s2 == 1 is bare too
        for a, b in MEDIA:
            gi, gt, gl = _grid(a, b)
            got = cd.run_interface(driver, a, b, gi, gt, gl, stack)
            assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), (thick, a, b)
    # the rule on a plain case: glass 1.7 -> 1.6 at 70 degrees through layers of 1.65 and 1.05: the 1.05 layer carries no wave
    ci = float(np.cos(np.radians(70.0)))
    ct = float(np.sqrt(1 - (1.7 / 1.6) ** 2 * (1 - ci * ci)))
    assert (1.7 / 1.05) ** 2 * (1 - ci * ci) > 1 > (1.7 / 1.65) ** 2 * (1 - ci * ci)
    bare = cd.run_interface(driver, 1.7, 1.6, ci, ct, 500.0, [])
    for stack in ([(1.65, 100.0), (1.05, 80.0)], [(1.05, 80.0)], [(1.65, 100.0), (2.0, 50.0), (1.05, 80.0)]):
        for forward in (True, False):
            assert _bits(cd.run_interface(driver, 1.7, 1.6, ci, ct, 500.0, stack, forward))[0] == _bits(bare)[0]
    assert _bits(cd.run_interface(driver, 1.7, 1.6, ci, ct, 500.0, [(1.65, 100.0)]))[0] != _bits(bare)[0]
    # no stack: the film entry, or bare -- interface_transmittance's bits
    tdrv = host_drivers.transmittance()
    for nc, l0 in ((0.0, 0.0), (1.38, 550.0)):
        assert _bits(cd.run_interface(driver, 1.0, 1.52, 0.8, 0.9, 500.0, [], film=(nc, l0)))[0] == \
            _bits(np.array([tdrv.ztr_interface(1.0, 1.52, 0.8, 0.9, nc, l0, 500.0)], F32))[0]


# ---- 4. equivalence with the single film --------------------------------------------------------------------------------------------
_LENS = {}


def _lens(cfg, oracle_lib):
    """the lens of a configuration and its ~10 k passing rays (no ray is left out), shared and read only"""
    if cfg not in _LENS:
        p, info, disp, surf, hs = tables(cfg)
        o, d = _rays(cfg, oracle_lib)
        _LENS[cfg] = dict(p=p, info=info, disp=disp, surf=surf, o=o, d=d, lam=_wavelengths(len(o)), L=gref.lens(info), h2=housings(info))
    return _LENS[cfg]


@pytest.mark.parametrize("cfg", CFGS)
def test_stack_q_is_the_single_film(cfg, driver, oracle_lib):
    """stack Q on every interface against set_coatings(1.38, 550) on every interface, path_transmittance over every ray: |dT| within
    the sum of the two paths' bounds (the film path's of test_transmittance_cpu.py, the stack path's below); with no stack, or layers
    all 0, the stack-aware path gives the film path's bits, coated and bare"""
    m = _lens(cfg, oracle_lib)
    count = len(m["surf"])
    tdrv = host_drivers.transmittance()
    film = (np.full(count, 1.38, F32), np.full(count, 550.0, F32))
    want = host_drivers.run_transmittance(tdrv, m["surf"], m["disp"], m["lam"], m["o"], m["d"], film)
    got = cd.run_transmittance(driver, m["surf"], m["disp"], m["lam"], m["o"], m["d"], [f32_pairs(Q)] * count)
    diff = float(np.abs(got.astype(np.float64) - want).max())
    print(cfg, "stack Q against the film: largest |dT| %.3e" % diff)
    assert (got > 0).all() and diff <= FILM_PATH_BOUND + 4 * max(PATH_MEASURED["forward"].values()), (cfg, diff)
    for fl in (None, film):
        plain = host_drivers.run_transmittance(tdrv, m["surf"], m["disp"], m["lam"], m["o"], m["d"], fl)
        for stacks in ([None] * count, [[]] * count):
            assert np.array_equal(_bits(cd.run_transmittance(driver, m["surf"], m["disp"], m["lam"], m["o"], m["d"], stacks, film=fl)), _bits(plain))


# ---- 5. physics ---------------------------------------------------------------------------------------------------------------------
def test_physics(driver):
    R = lambda *a, **k: 1.0 - float(cd.run_interface(driver, *a, **k)[0])  # noqa: E731
    worst = max(BOUND.values())
    # a half-wave layer at lambda and normal incidence is absent
    for n1, n2 in ((1.0, 1.52), (1.8, 1.0), (1.65, 1.5)):
        bare = R(n1, n2, 1.0, 1.0, 550.0, [])
        for nj in (1.38, 2.05, 4.0):
            half = [(nj, 550.0 / (2 * nj))]
            assert abs(R(n1, n2, 1.0, 1.0, 550.0, f32_pairs(half)) - bare) <= BOUND["THICK"], (n1, n2, nj)
    # a quarter-quarter pair with n_a^2 n_s = n_b^2 n_0 reflects nothing at lambda0 (n_a next to n_0, met first)
    n0, ns, na = 1.0, 1.52, 1.38
    nb = na * np.sqrt(ns / n0)
    pair = f32_pairs([(na, 550.0 / (4 * na)), (nb, 550.0 / (4 * nb))])
    assert R(n0, ns, 1.0, 1.0, 550.0, pair) <= BOUND["QHQ"]
    assert R(ns, n0, 1.0, 1.0, 550.0, pair, forward=False) <= BOUND["QHQ"]         # the same layers from the glass side
    assert R(n0, ns, 1.0, 1.0, 450.0, pair) > 10 * BOUND["QHQ"]
    # QHQ reflects less than Q at 450, 550 and 650 nm on air -> 1.52, and both less than the bare 4.26 %: the issue's table
    table = {}
    for lam in (450.0, 550.0, 650.0):
        bare, q, qhq = R(1.0, 1.52, 1.0, 1.0, lam, []), R(1.0, 1.52, 1.0, 1.0, lam, f32_pairs(Q)), R(1.0, 1.52, 1.0, 1.0, lam, f32_pairs(QHQ))
        table[lam] = (bare, q, qhq)
        assert qhq + worst < q < bare - worst, table
    print({k: ["%.4f %%" % (100 * v) for v in t] for k, t in table.items()})
    for lam, (q, qhq) in {450.0: (0.0162, 0.0021), 550.0: (0.0126, 0.0018), 650.0: (0.0144, 0.0003)}.items():
        assert abs(table[lam][0] - 0.0426) < 5e-5 and abs(table[lam][1] - q) < 5e-5 and abs(table[lam][2] - qhq) < 5e-5, (lam, table[lam])
    # reciprocity of one interface: the same reflectance from the other side, the layers met backwards
    for stack in (f32_pairs(QHQ), f32_pairs(R8)):
        ci = F32(0.8)
        ct = F32(np.sqrt(1 - (1.0 / 1.52) ** 2 * (1 - 0.64)))
        a = R(1.0, 1.52, ci, ct, 500.0, stack)
        b = R(1.52, 1.0, ct, ci, 500.0, stack, forward=False)
        assert abs(a - b) <= 2 * BOUND["R8"]


# ---- 6. the paths -------------------------------------------------------------------------------------------------------------------
def _stacks(disp, which):
    """FILE-order stacks for a camera and the same in trace order for the drivers and the restatement"""
    file_order = cr.stacks_where_media_differ(disp, NAMED[which])
    return file_order, cr.to_trace_order(file_order)


_FORWARD = {}


def _forward(cfg, which, driver, oracle_lib):
    key = (cfg, which)
    if key not in _FORWARD:
        m = _lens(cfg, oracle_lib)
        _, trace = _stacks(m["disp"], which)
        with cr.in_force(trace, m["disp"]):
            ref, ok = tref.transmittance(m["surf"], m["disp"], m["lam"], m["o"], m["d"], *cr.marked_films(trace))
        assert ok.all()
        got = cd.run_transmittance(driver, m["surf"], m["disp"], m["lam"], m["o"], m["d"], trace)
        assert (got > 0).all() and (got <= 1).all()
        _FORWARD[key] = float(np.abs(got.astype(np.float64) - ref).max()), float(np.median(ref))
    return _FORWARD[key]


@pytest.mark.parametrize("cfg", CFGS)
def test_forward_path_against_f64(cfg, driver, oracle_lib):
    """path_transmittance under QHQ and under R8 on every interface between unequal media, every ray"""
    errs = {w: _forward(cfg, w, driver, oracle_lib) for w in ("QHQ", "R8")}
    print(cfg, "forward:", {w: "%.3e (median T %.4f)" % e for w, e in errs.items()})
    worst = max(e[0] for e in errs.values())
    assert PATH_MEASURED["forward"][cfg] / 4 <= worst <= 4 * PATH_MEASURED["forward"][cfg], (cfg, errs)
    assert errs["QHQ"][1] > 0.85         # the three-layer stack: lenses that pass 0.53 to 0.69 bare (test_transmittance_cpu.py)


def _four_pairs(cam_pairs):
    k = len(cam_pairs)
    return cam_pairs[[0, k // 3, (2 * k) // 3, k - 1]]


@pytest.mark.parametrize("cfg", CFGS)
def test_ghosts_against_f64(cfg, driver, oracle_lib):
    """ghost_trace for four pairs of ghost_pairs() under QHQ and under R8: the weights of the ghosts both trace (f64 margin at least
    MARGIN) against the restatement; origin, dir and flags are the no-stack call's bits"""
    m = _lens(cfg, oracle_lib)
    cam = ZoicCamera(device=-1)
    cam.update(**m["p"])
    pairs = _four_pairs(cam.ghost_pairs())
    cam.close()
    gdrv = host_drivers.ghost()
    plain = host_drivers.run_ghost_records(gdrv, m["L"], m["disp"], m["lam"], m["o"], m["d"], pairs)
    worst, compared = {}, 0
    for which in ("QHQ", "R8"):
        _, trace = _stacks(m["disp"], which)
        got = cd.run_ghost_records(driver, m["L"], m["disp"], m["lam"], m["o"], m["d"], pairs, trace)
        assert np.array_equal(_bits(got[..., 0:6]), _bits(plain[..., 0:6])) and np.array_equal(_bits(got[..., 7]), _bits(plain[..., 7]))
        assert not np.array_equal(_bits(got[..., 6]), _bits(plain[..., 6]))
        err = 0.0
        with cr.in_force(trace, m["disp"]):
            for j, (a, b) in enumerate(pairs):
                ref = gref.ghost(m["L"], m["disp"], m["lam"], m["o"], m["d"], int(a), int(b), *cr.marked_films(trace))
                go, gd, gw, flags, reason, iface, leg = split(got[:, j])
                both = (ref["margin"] >= MARGIN) & (reason == 0) & (ref["reason"] == 0)
                compared += int(both.sum())
                if both.any():
                    err = max(err, float(np.abs(gw[both] - ref["weight"][both]).max()))
                    assert (gw[both] > 0).all() and (gw[both] <= 1).all()
        worst[which] = err
    print(cfg, "ghost weights:", {k: "%.3e" % v for k, v in worst.items()}, "compared", compared)
    assert compared >= 1000
    assert PATH_MEASURED["ghost"][cfg] / 4 <= max(worst.values()) <= 4 * PATH_MEASURED["ghost"][cfg], (cfg, worst)
    # the plain path under the stacks is path_transmittance's weight: the ghost tracer and the forward trace price one lens
    _, trace = _stacks(m["disp"], "QHQ")
    w = cd.run_ghost_records(driver, m["L"], m["disp"], m["lam"], m["o"], m["d"], None, trace)[:, 0, 6]
    t = cd.run_transmittance(driver, m["surf"], m["disp"], m["lam"], m["o"], m["d"], trace, housing2=m["h2"])
    live = (w > 0) & (t > 0)
    assert live.mean() > 0.98 and np.abs(w[live].astype(np.float64) - t[live]).max() <= 4 * max(PATH_MEASURED["forward"].values())


_BACK = {}


def _back(cfg, which, oracle_lib):
    """zoic_trace_back_ray_transmittance and its spectral form on the lens's forward records under the stacks, against the restatement"""
    key = (cfg, which)
    if key not in _BACK:
        L = tr.lens(oracle_lib, cfg)
        file_order, trace = _stacks(L.disp, which)
        tr.coat(L.cam, None)
        L.cam.set_coating_stacks(None)
        base = {lam: tr.lib_throughput(L.cam, L.o, L.d, lam) for lam in (None, 486.1327)}
        L.cam.set_coating_stacks(file_order)
        R = tr.Throughput(L.info, L.p, L.disp, cr.marked_films(trace))
        out = {}
        with cr.in_force(trace, L.disp):
            for lam in (None, 486.1327):
                ref = R.trace(L.o, L.d) if lam is None else R.trace_at(L.o, L.d, lam)
                edge, T64 = R.edge(ref), R.transmittance(L.o, L.d, lam)
                ps, fl, T = tr.lib_throughput(L.cam, L.o, L.d, lam)
                assert np.array_equal(_bits(ps), _bits(base[lam][0])) and np.array_equal(fl, base[lam][1])      # Ps and flags: the no-stack call's
                assert not np.array_equal(_bits(T), _bits(base[lam][2]))
                out[lam] = ref, edge, T64, fl, T
            Tf, passes = tr.forward_transmittance(L.info, L.disp, L.o0, L.d0, tr.LAMBDA_D32, cr.marked_films(trace))
        L.cam.set_coating_stacks(None)
        _BACK[key] = out, Tf, passes
    return _BACK[key]


@pytest.mark.parametrize("cfg", CFGS)
def test_trace_back_against_f64_and_reciprocity(cfg, oracle_lib):
    worst, e_rec, recip = {}, 0.0, 0.0
    for which in ("QHQ", "R8"):
        out, Tf, passes = _back(cfg, which, oracle_lib)
        err = 0.0
        for lam, (ref, edge, T64, fl, T) in out.items():
            both = ~edge & ((fl & 1) == 1)
            assert both.sum() >= 2048 and (T[both] > 0).all() and (T[both] <= 1).all() and (_bits(T[(fl & 1) == 0]) == 0).all()
            err = max(err, float(np.abs(T.astype(np.float64) - T64)[both].max()))
        worst[which] = err
        ref, edge, T64, fl, T = out[None]            # the d-line records are the path: forward T of the start against backward T
        both = ~edge & ((fl & 1) == 1)
        assert passes[both].all()
        e_rec = max(e_rec, float(np.abs(T64 - Tf)[both].max()))
        recip = max(recip, float(np.abs(T.astype(np.float64) - Tf)[both].max()))
    print(cfg, "trace-back:", {k: "%.3e" % v for k, v in worst.items()}, "E_rec %.3e, |T_host_back - T_fwd_f64| %.3e" % (e_rec, recip))
    assert PATH_MEASURED["back"][cfg] / 4 <= max(worst.values()) <= 4 * PATH_MEASURED["back"][cfg], (cfg, worst)
    assert e_rec <= 4 * E_REC
    assert recip <= 4 * PATH_MEASURED["back"][cfg] + e_rec


@pytest.mark.parametrize("spectral", [False, True], ids=["d-line", "spectral"])
@pytest.mark.parametrize("cfg", CFGS)
def test_splat_side_against_f64(cfg, spectral, oracle_lib):
    """zoic_splat_point_transmittance[_spectral] under the stacks: the ray side's bits on the rays rebuilt from the recorded aims
    (origin P, dir P - A in float32), and within the trace-back bound of the restatement of those rays"""
    p = tc.params_of(cfg)
    cam = bs.set_dispersion(tc.update(ZoicCamera(device=-1), p), cfg)
    info, disp = cam.info(), cam.dispersion()
    file_order, trace = _stacks(disp, "QHQ")
    file_order[-1 - int(np.flatnonzero([bool(s) for s in trace])[0])] = R8         # one interface carries the eight layers
    trace = cr.to_trace_order(file_order)
    cam.set_coating_stacks(file_order)
    R = tr.Throughput(info, p, disp, cr.marked_films(trace))
    pts = pc.points(p)
    lam = pc.wavelengths(len(pts)) if spectral else [None] * len(pts)
    z = F32(cam.pupil_square()[0])
    u = np.random.default_rng(77).random((len(pts), 8, 2)).astype(F32)
    worst, traced = 0.0, 0
    with cr.in_force(trace, disp):
        for i, P in enumerate(pts):
            b = cam.pupil_bounds_point(P, 16)
            rec = cam.splat_point(P, b, u[i], lam[i])
            T = cam.splat_point_transmittance(P, b, u[i], lam[i])
            go = rec["flags"] != _capi.SPLAT_NO_BOX
            assert np.array_equal(T > 0, (rec["flags"] & 1) == 1) and (_bits(T[~(T > 0)]) == 0).all() and (T <= 1).all()
            if not go.any():
                continue
            with np.errstate(invalid="ignore"):
                A = np.stack([rec["ax"][go], rec["ay"][go], np.full(go.sum(), z, F32)], 1).astype(F32)
                o = np.repeat(np.asarray(P, F32)[None, :], go.sum(), 0)
                d = (o - A).astype(F32)
            ps, fl, want = tr.lib_throughput(cam, o, d, lam[i])
            assert np.array_equal(_bits(want), _bits(T[go])), (cfg, i)
            ok = (fl & 1) == 1
            if ok.any() and (lam[i] is None or bs.valid(np.array([lam[i]], F32))[0]):
                ref = R.trace(o, d) if lam[i] is None else R.trace_at(o, d, lam[i])
                both = ok & ~R.edge(ref)
                T64 = R.transmittance(o, d, lam[i])
                if both.any():
                    worst = max(worst, float(np.abs(want.astype(np.float64) - T64)[both].max()))
                    traced += int(both.sum())
    print(cfg, "splat side: compared %d, largest |T_host - T_f64| %.3e" % (traced, worst))
    assert traced >= 20 or cfg == "C4"      # (the points are placed for C3's field: none of C4's aims is traced off the edge set)
    assert worst <= 4 * PATH_MEASURED["back"][cfg]
    cam.close()


def test_measured_figures_are_the_recorded_ones():
    """no placeholder is left: every recorded figure is a measured, positive one"""
    assert all(v > 0 for d in PATH_MEASURED.values() for v in d.values()) and E_REC > 0 and all(v > 0 for v in MEASURED.values())


# ---- 7. resources -------------------------------------------------------------------------------------------------------------------
def test_stack_kernels_budget():
    """the four stack-aware kernels against their plain twins: 0 scratch, 0 VGPR spills, no LDS beyond the twin's, VGPRs within the twin's
    stated cap (128 for transmittance and ghosts, 96 for the trace-back ray side, the RAYTRACED splat kernel's 79 for its splat side), and
    -- the trace-back twins' own budget -- no SGPR spill on the trace-back side.  Their names avoid the substrings the other budget
    tests count kernels by.

    Measured (VGPRs, SGPR spills): loss 109, flare 109, tb_stack 57 / 0, aim_stack 55 / 0 (it takes one slab per launch: under the plain
    kernel's grid-stride walk it spilled two scalar registers)."""
    res = kernel_resources()
    twins = {"kolb_stack_loss_kernel": ("kolb_transmittance_kernel", 128), "kolb_stack_flare_kernel": ("kolb_ghost_kernel", 128),
             "tb_stack_throughput_kernel": ("tb_throughput_kernel<1>", 96), "aim_stack_throughput_kernel": ("aim_throughput_kernel<1>", 79)}
    for name, (twin, cap) in twins.items():
        mine = [v for k, v in res.items() if name in k]
        theirs = [v for k, v in res.items() if k.split("::")[-1].startswith(twin)]
        assert len(mine) == 1 and len(theirs) == 1, (name, sorted(res))
        v, t = mine[0], theirs[0]
        print(name, v)
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] <= t["lds"] and v["kernarg"] <= 4096, (name, v)
        assert v["vgpr"] + v["agpr"] <= cap, (name, v)
        if "throughput" in name:
            assert v["sgpr_spill"] == 0, (name, v)
        for word in ("transmittance", "splat", "ghost", "pupil_bounds", "differentials_kernel", "spectral", "trace_back", "hero",
                     "tb_throughput_kernel", "aim_throughput_kernel"):
            assert word not in name, (name, word)

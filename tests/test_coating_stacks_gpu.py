"""Multilayer coatings on the device: the four stack-aware kernels against the host build of csrc/coating_stack.hpp, bit for bit, on C2
and C3 with QHQ on the glass-air interfaces and R8 on one, at n = 1, 63, 65 and 4096 + 37 -- zoic_ray_transmittance_device (d-line, a
wavelength per ray, hero k = 3), zoic_create_ghost_rays_device (4 pairs), the trace-back and the splat transmittance against their
host calls -- and a setter sequence on one camera.  The inputs and starts are hero_cases.loss_reference's 4096 rows; the 37 rows past
them repeat the first 37 (every row carries its own sample, wavelength and stream state)."""
import numpy as np
import pytest

from zoic_amd import PRECISION_STRICT, ZoicCamera, pupil_bounds_records

import backward_spectral_ref as bs
import coating_stack_drivers as cd
import coating_stack_ref as cr
import differentials_ref as dref
import ghost_ref as gref
import hero_cases as hr
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr
from coating_stack_ref import QHQ, R8
from device_cases import bits_f32 as _bits
from hero_cases import LOSS_CAMERAS as CAMERAS, loss_reference as _reference
from spectral_ref import LAMBDA_D32
from transmittance_ref import films_where_media_differ, housings

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 63, 65, 4096 + 37]
_TABLES = {}


@pytest.fixture(scope="module")
def driver():
    return cd.driver()


def _stacks_for(disp):
    """FILE-order stacks: QHQ on every interface between unequal media, R8 on the rearmost of them; and the same in trace order"""
    first = int(np.flatnonzero(disp["ior_d"] != np.append(disp["ior_d"][1:], F32(1.0)))[0])
    file_order = cr.stacks_where_media_differ(disp, QHQ, special={first: R8})
    return file_order, cr.to_trace_order(file_order)


def _tables(name):
    if name not in _TABLES:
        cam = hr.spec(name).camera(device=-1)
        info, disp, pairs = cam.info(), cam.dispersion(), cam.ghost_pairs()
        cam.close()
        file_order, trace = _stacks_for(disp)
        k = len(pairs)
        _TABLES[name] = dict(disp=disp, surf=dref.surfaces(info), h2=housings(info), L=gref.lens(info), file=file_order, trace=trace,
                             pairs=pairs[[0, k // 3, (2 * k) // 3, k - 1]], film=films_where_media_differ(disp))
    return _TABLES[name]


def _rows(a, n):
    """the first n rows of the 4096, the rows past them repeating the first ones"""
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def _expected_t(driver, t, stacks, starts, here, weights, film=None):
    n, k = here.shape
    want = np.zeros((n, k), F32)
    for j in range(k):
        rows = np.nonzero((weights[:, j] != 0) & hr.valid(here[:, j]))[0]
        if len(rows):
            if stacks is None:
                import host_drivers
                want[rows, j] = host_drivers.run_transmittance(host_drivers.transmittance(), t["surf"], t["disp"], here[rows, j], starts[rows, 0:3],
                                                               starts[rows, 3:6], film, t["h2"])
            else:
                want[rows, j] = cd.run_transmittance(driver, t["surf"], t["disp"], here[rows, j], starts[rows, 0:3], starts[rows, 3:6], stacks,
                                                     film=film, housing2=t["h2"])
    return want


def _forward(cam, s, lam, st):
    import torch
    ts, tl = torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(lam)).cuda()
    tst = torch.from_numpy(np.array(st).view(np.int32)).cuda()
    return ts, tl, tst, cam.create_rays_hero(ts, tl, rng_states=tst)["rays"]


# ---- 8. transmittance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["d-line", "spectral", "hero3"])
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_transmittance_equals_the_host_build(gpu, oracle_lib, driver, cfg, form):
    import torch
    name = CAMERAS[cfg]
    k = 3 if form == "hero3" else 1
    lam_all = np.full((hr.N, 1), LAMBDA_D32, F32) if form == "d-line" else None
    s, lam, st, words, starts = _reference(oracle_lib, name, k, lam=lam_all, key="d-line" if form == "d-line" else None)
    t = _tables(name)
    cam = hr.spec(name).camera(precision=PRECISION_STRICT)
    cam.set_coating_stacks(t["file"])
    live_seen = lost = 0
    for n in SIZES:
        ts, tl, tst, rays = _forward(cam, _rows(s, n), _rows(lam, n), _rows(st, n))
        if form == "d-line":
            got = cam.transmittance(ts, rays.view(n, 8), rng_states=tst)
        else:
            got = cam.transmittance(ts, rays if k > 1 else rays.view(n, 8), wavelengths=tl if k > 1 else tl.view(n), rng_states=tst)
        torch.cuda.synchronize()
        g = got.cpu().numpy().reshape(n, k)
        r = rays.cpu().numpy().reshape(n, k, 8)
        assert hr.same_words(r.view(np.uint32), _rows(words, n)).all()
        want = _expected_t(driver, t, t["trace"], _rows(starts, n), _rows(lam, n), r[:, :, 6])
        assert np.array_equal(_bits(g), _bits(want)), (cfg, form, n, np.argwhere(_bits(g) != _bits(want))[:8].tolist())
        live = (r[:, :, 6] != 0) & hr.valid(_rows(lam, n))
        assert (g[live] > 0).all() and (g <= 1).all() and not _bits(g[~live]).any()
        live_seen += int(live.sum())
        lost += int(((r[:, :, 7].view(np.uint32) >> 8) & 1).sum())
    assert live_seen >= 1000 * k
    print(cfg, form, "live columns", live_seen, "lost companions", lost)
    cam.close()


# ---- 9. ghosts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_ghosts_equal_the_host_records(gpu, oracle_lib, driver, cfg):
    import torch
    name = CAMERAS[cfg]
    s, lam, st, words, starts = _reference(oracle_lib, name, 1)
    t = _tables(name)
    cam = hr.spec(name).camera(precision=PRECISION_STRICT)
    cam.set_coating_stacks(t["file"])
    traced = 0
    for n in SIZES:
        ts, tl, tst, rays = _forward(cam, _rows(s, n), _rows(lam, n), _rows(st, n))
        rays = rays.view(n, 8)
        r = rays.cpu().numpy()
        assert hr.same_words(r.view(np.uint32).reshape(n, 1, 8), _rows(words, n)).all()
        got = cam.create_ghost_rays(ts, rays, t["pairs"], wavelengths=tl.view(n), rng_states=tst)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        st_n = _rows(starts, n)
        want = cd.run_ghost_records(driver, t["L"], t["disp"], _rows(lam, n)[:, 0], st_n[:, 0:3], st_n[:, 3:6], t["pairs"], t["trace"], have=r[:, 6] != 0)
        assert np.array_equal(_bits(g), _bits(want)), (cfg, n, np.argwhere(_bits(g) != _bits(want))[:8].tolist())
        traced += int((_bits(g[..., 7]) == 1).sum())
    assert traced >= 1000
    cam.close()


# ---- 10. trace-back transmittance -----------------------------------------------------------------------------------------------------
def _backward_camera(cfg, device):
    p = tc.params_of(cfg)
    cam = bs.set_dispersion(tc.update(ZoicCamera(device=device), p), cfg)
    return cam, p, _stacks_for(cam.dispersion())[0]


def _records(cam, n):
    from zoic_amd.workloads import ray_rng_states, synthetic_samples
    m = 4096
    fwd = cam.create_rays(synthetic_samples(m, 64, 64, 1), rng_states=ray_rng_states(m))
    rec = np.ascontiguousarray(fwd["rays"]).view(F32).reshape(-1, 8)
    return _rows(rec, n)


@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_trace_back_transmittance_equals_the_host_call(gpu, cfg):
    cam, p, file_order = _backward_camera(cfg, 0)
    cam.set_coating_stacks(file_order)
    all_rays = _records(cam, SIZES[-1])
    all_lam = bs.mixed_wavelengths(SIZES[-1])
    traced = 0
    for n in SIZES:
        rays, lam = all_rays[:n], all_lam[:n]
        for w in (None, lam):
            T, scr, fl = cam.trace_back_transmittance(rays, wavelengths=w)
            ps, hf, hT = tr.lib_throughput(cam, rays[:, 0:3], rays[:, 3:6], w)
            assert np.array_equal(_bits(T), _bits(hT)), (cfg, n, w is not None)
            s2, f2 = cam.trace_back(rays, wavelengths=w)
            assert np.array_equal(scr.view(np.uint32), s2.view(np.uint32)) and np.array_equal(fl, f2)
            assert np.array_equal(scr.view(np.uint32), ps.view(np.uint32)) and np.array_equal(fl.astype(np.uint32), hf)
            traced += int((hf & 1).sum())
    assert traced >= 2048
    # the stacks count: the same rays without them
    bare = cam.trace_back_transmittance(all_rays)[0]
    cam.set_coating_stacks(None)
    assert not np.array_equal(_bits(cam.trace_back_transmittance(all_rays)[0]), _bits(bare))
    cam.close()


# ---- 11. splat transmittance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C2", "C3"])
def test_splat_transmittance_equals_the_host_call(gpu, cfg):
    import torch
    cam, p, file_order = _backward_camera(cfg, 0)
    cam.set_coating_stacks(file_order)
    n, m = 257, 8
    pts = pc.batch(p, n)
    u = np.random.default_rng(257 * 8).random((n, m, 2)).astype(F32)
    lam = np.resize(pc.wavelengths(10), n).astype(F32)
    dev = torch.device("cuda", 0)
    P, U = torch.from_numpy(pts).to(dev), torch.from_numpy(u).to(dev)
    bounds = cam.pupil_bounds(P, 16)
    b = pupil_bounds_records(bounds)
    empty = np.flatnonzero(b["count"] == 0)
    assert len(empty) >= 1                                   # a point with an empty box
    for w in (None, lam):
        T = cam.splat_transmittance(P, bounds, U, None if w is None else torch.from_numpy(w).to(dev))
        torch.cuda.synchronize()
        g = T.cpu().numpy()
        assert g.shape == (n, m) and (_bits(g[empty]) == 0).all() and (g > 0).sum() >= n
        for i in range(n):
            host = cam.splat_point_transmittance(pts[i], b[i:i + 1], u[i], None if w is None else w[i])
            assert np.array_equal(_bits(host), _bits(g[i])), (cfg, i, w is not None)
    cam.close()


@pytest.mark.parametrize("shape", [(174763, 3), (2, (1 << 19) + 5)], ids=["grid-plus-one", "m-past-a-slab"])
def test_splat_transmittance_past_one_slab(gpu, shape):
    """the stack-aware splat kernel takes one slab of 2048 x 256 items per launch: a batch of one slab and one item (the boundary falls
    inside a point: 524288 = 174762 x 3 + 2), and two points of more aims than a slab holds (the boundary inside the first point, the
    point index by comparison, not division) -- against the same call on the two halves of the points, each within slabs of its own,
    and against the host call on points either side of every boundary"""
    import torch
    n, m = shape
    cam, p, file_order = _backward_camera("C3", 0)
    cam.set_coating_stacks(file_order)
    base = pc.batch(p, 64)
    pts = np.ascontiguousarray(base[np.arange(n) % len(base)])
    rng = np.random.default_rng(n + m)
    u = rng.random((n, m, 2), dtype=F32)
    lam = np.resize(pc.wavelengths(10), n).astype(F32)
    dev = torch.device("cuda", 0)
    P, U, L = torch.from_numpy(pts).to(dev), torch.from_numpy(u).to(dev), torch.from_numpy(lam).to(dev)
    bounds = cam.pupil_bounds(P, 16)
    T = cam.splat_transmittance(P, bounds, U, L)
    h = n // 2
    A = cam.splat_transmittance(P[:h], bounds[:h], U[:h], L[:h])
    B = cam.splat_transmittance(P[h:], bounds[h:], U[h:], L[h:])
    torch.cuda.synchronize()
    assert n * m > 2048 * 256 and (n * m) % (2048 * 256) != 0
    assert torch.equal(T.view(torch.int32), torch.cat([A, B]).view(torch.int32))
    g = T.cpu().numpy()
    assert (g > 0).sum() >= n * m // 8 and (g <= 1).all()
    b = pupil_bounds_records(bounds)
    edge = (2048 * 256) // m
    for i in sorted({0, n - 1} | {k for k in (edge - 1, edge, edge + 1) if 0 <= k < n}):
        host = cam.splat_point_transmittance(pts[i], b[i:i + 1], u[i], lam[i])
        assert np.array_equal(_bits(host), _bits(g[i])), (shape, i)
    cam.close()


# ---- 12. the setter sequence ----------------------------------------------------------------------------------------------------------
def test_setter_sequence_on_one_camera(gpu, oracle_lib, driver):
    """stacks set, cleared, set again (others), then an update of the same lens: after each step the device call equals the host build
    for the table then in force; cleared, it gives the single film's bits"""
    import torch
    name = CAMERAS["C2"]
    s, lam, st, words, starts = _reference(oracle_lib, name, 1)
    t = _tables(name)
    n = 4096
    sp = hr.spec(name)
    cam = sp.camera(precision=PRECISION_STRICT)
    cam.set_coatings(t["film"][0][::-1], t["film"][1][::-1])
    ts, tl, tst, rays = _forward(cam, s, lam, st)
    rays = rays.view(n, 8)
    w = rays.cpu().numpy()[:, 6:7]
    back = _rows(rays.cpu().numpy(), 512)

    def check(stacks_trace, label):
        got = cam.transmittance(ts, rays, wavelengths=tl.view(n), rng_states=tst)
        torch.cuda.synchronize()
        want = _expected_t(driver, t, stacks_trace, starts, lam, w, film=t["film"])
        assert np.array_equal(_bits(got.cpu().numpy().reshape(n, 1)), _bits(want)), label
        T = cam.trace_back_transmittance(back)[0]
        assert np.array_equal(_bits(T), _bits(tr.lib_throughput(cam, back[:, 0:3], back[:, 3:6])[2])), label
        return got.cpu().numpy()

    film_only = check(None, "film only")
    cam.set_coating_stacks(t["file"])
    first = check(t["trace"], "set")
    assert not np.array_equal(_bits(first), _bits(film_only))
    cam.set_coating_stacks(None)
    assert np.array_equal(_bits(check(None, "cleared")), _bits(film_only))            # the single-film bits
    other_file = cr.stacks_where_media_differ(t["disp"], R8)
    cam.set_coating_stacks(other_file)
    second = check(cr.to_trace_order(other_file), "set again")
    assert not np.array_equal(_bits(second), _bits(first))
    cam.update(**sp.params)                                                            # the same lens: the override stays in force
    assert np.array_equal(_bits(check(cr.to_trace_order(other_file), "after an update")), _bits(second))
    half = [st_ if i % 2 else None for i, st_ in enumerate(t["file"])]                 # layers == 0 leaves the film entry in force
    cam.set_coating_stacks(half)
    check(cr.to_trace_order(half), "every other interface")
    cam.close()

"""The Python binding's argument rules on the MI355X: every tensor argument of every torch-path call of zoic_amd/camera.py is refused
with ValueError when its dtype, its shape, its layout or its device is wrong -- in Python, before any launch: result buffers filled
with a sentinel beforehand hold their bits afterwards -- and a call that is given out / flags / jacobian buffers writes into them the
bits of the same call without them.

One camera (the double Gauss with its dispersion table), n = 5 samples / points / rays, k = 2 hero wavelengths, m = 1 aim per point
and one ghost pair: the smallest shapes at which a mixed-up dimension still shows."""
import numpy as np
import pytest

from zoic_amd import ZoicCamera
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import pupil_cases as pc
import traceback_cases as tc

pytestmark = pytest.mark.gpu

N, K, M = 5, 2, 1
SENTINEL = 0x7FA51234   # a NaN with a payload no kernel writes


class _Setup:
    """the camera and one well-formed value for every tensor argument (device tensors, read only)"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        p = pc.params_of("C3")
        self.cam = tc.update(ZoicCamera(device=0), p)
        bs.set_dispersion(self.cam, pc.CAMERAS["C3"][0])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
        cam = self.cam
        lam = np.array([[450.0, 640.0], [500.0, 587.5618], [550.0, 420.0], [600.0, 700.0], [650.0, 480.0]], np.float32)
        a = dict(samples=up(synthetic_samples(N, 64, 36, 1, seed=3)), rng_states=up(ray_rng_states(N, seed=3).view(np.int32)),
                 wavelengths=up(lam[:, 0]), hero_wavelengths=up(lam), points=up(pc.points(p)[:N]),
                 u=up(np.random.default_rng(5).random((N, M, 2)).astype(np.float32)))
        a["rays"] = cam.create_rays(a["samples"], rng_states=a["rng_states"])["rays"]
        a["spectral_rays"] = cam.create_rays(a["samples"], rng_states=a["rng_states"], wavelengths=a["wavelengths"])["rays"]
        a["hero_rays"] = cam.create_rays_hero(a["samples"], a["hero_wavelengths"], rng_states=a["rng_states"])["rays"]
        a["bounds"] = cam.pupil_bounds(a["points"])
        torch.cuda.synchronize(self.dev)
        assert (a["rays"][:, 6] > 0).any() and (a["bounds"].view(torch.int32)[:, 8] > 0).any()
        self.args = a
        self.pairs = cam.ghost_pairs()[:1]
        assert self.pairs.shape == (1, 2)


@pytest.fixture(scope="module")
def setup(gpu):
    s = _Setup()
    yield s
    s.cam.close()


def _rays_dict(t):
    return None if t is None else dict(rays=t)


# name -> (call(cam, a, pairs) with a the dict of its tensor arguments (a result buffer may be None),
#          the arguments read: name in the call -> name in the setup; the first one is the item that sets n,
#          the result buffers: name -> (shape, integer?))
CALLS = {
    "create_rays": (lambda c, a, _: c.create_rays(a["samples"], rng_states=a["rng_states"], ray_index_base=7, out=_rays_dict(a["out"])),
                    dict(samples="samples", rng_states="rng_states"), dict(out=((N, 8), False))),
    "create_rays(wavelengths=)": (lambda c, a, _: c.create_rays(a["samples"], rng_states=a["rng_states"], out=_rays_dict(a["out"]),
                                                                wavelengths=a["wavelengths"]),
                                  dict(samples="samples", wavelengths="wavelengths", rng_states="rng_states"), dict(out=((N, 8), False))),
    "create_rays_hero": (lambda c, a, _: c.create_rays_hero(a["samples"], a["wavelengths"], rng_states=a["rng_states"], out=_rays_dict(a["out"])),
                         dict(samples="samples", wavelengths="hero_wavelengths", rng_states="rng_states"), dict(out=((N, K, 8), False))),
    "create_rays_resident": (lambda c, a, _: c.create_rays_resident(a["samples"], ray_index_base=7, out=a["out"]),
                             dict(samples="samples"), dict(out=((N, 8), False))),
    "project_points": (lambda c, a, _: c.project_points(a["points"], out=a["out"], flags=a["flags"]),
                       dict(points="points"), dict(out=((N, 2), False), flags=((N,), True))),
    "project_points(wavelengths=)": (lambda c, a, _: c.project_points(a["points"], out=a["out"], flags=a["flags"], wavelengths=a["wavelengths"]),
                                     dict(points="points", wavelengths="wavelengths"), dict(out=((N, 2), False), flags=((N,), True))),
    "trace_back": (lambda c, a, _: c.trace_back(a["rays"], out=a["out"], flags=a["flags"]),
                   dict(rays="rays"), dict(out=((N, 2), False), flags=((N,), True))),
    "trace_back(wavelengths=)": (lambda c, a, _: c.trace_back(_rays_dict(a["rays"]), out=a["out"], flags=a["flags"], wavelengths=a["wavelengths"]),
                                 dict(rays="spectral_rays", wavelengths="wavelengths"), dict(out=((N, 2), False), flags=((N,), True))),
    "trace_back_jacobian": (lambda c, a, _: c.trace_back_jacobian(a["rays"], out=a["out"], flags=a["flags"], jacobian=a["jacobian"]),
                            dict(rays="rays"), dict(out=((N, 2), False), flags=((N,), True), jacobian=((N, 2, 6), False))),
    "trace_back_jacobian(wavelengths=)": (lambda c, a, _: c.trace_back_jacobian(a["rays"], a["wavelengths"], a["out"], a["flags"], a["jacobian"]),
                                          dict(rays="spectral_rays", wavelengths="wavelengths"),
                                          dict(out=((N, 2), False), flags=((N,), True), jacobian=((N, 2, 6), False))),
    "pupil_bounds": (lambda c, a, _: c.pupil_bounds(a["points"], out=a["out"]), dict(points="points"), dict(out=((N, 12), False))),
    "pupil_bounds(wavelengths=)": (lambda c, a, _: c.pupil_bounds(a["points"], 8, pc.WINDOW, a["wavelengths"], out=a["out"]),
                                   dict(points="points", wavelengths="wavelengths"), dict(out=((N, 12), False))),
    "splat_points": (lambda c, a, _: c.splat_points(a["points"], a["bounds"], a["u"], out=a["out"]),
                     dict(points="points", bounds="bounds", u="u"), dict(out=((N, M, 8), False))),
    "splat_points(wavelengths=)": (lambda c, a, _: c.splat_points(a["points"], a["bounds"], a["u"], a["wavelengths"], out=a["out"]),
                                   dict(points="points", bounds="bounds", u="u", wavelengths="wavelengths"), dict(out=((N, M, 8), False))),
    "ray_differentials": (lambda c, a, _: c.ray_differentials(a["samples"], a["rays"], rng_states=a["rng_states"], out=a["out"]),
                          dict(samples="samples", rays="rays", rng_states="rng_states"), dict(out=((N, 12), False))),
    "ray_differentials(wavelengths=)": (lambda c, a, _: c.ray_differentials(a["samples"], _rays_dict(a["rays"]), 0.5, 0.25, a["rng_states"], out=a["out"],
                                                                            wavelengths=a["wavelengths"], chromatic=True),
                                        dict(samples="samples", rays="spectral_rays", rng_states="rng_states", wavelengths="wavelengths"),
                                        dict(out=((N, 12), False))),
    "transmittance": (lambda c, a, _: c.transmittance(a["samples"], a["rays"], rng_states=a["rng_states"], out=a["out"]),
                      dict(samples="samples", rays="rays", rng_states="rng_states"), dict(out=((N,), False))),
    "transmittance(wavelengths=)": (lambda c, a, _: c.transmittance(a["samples"], a["rays"], a["wavelengths"], a["rng_states"], out=a["out"]),
                                    dict(samples="samples", rays="spectral_rays", wavelengths="wavelengths", rng_states="rng_states"),
                                    dict(out=((N,), False))),
    "transmittance(hero)": (lambda c, a, _: c.transmittance(a["samples"], _rays_dict(a["rays"]), a["wavelengths"], a["rng_states"], out=a["out"]),
                            dict(samples="samples", rays="hero_rays", wavelengths="hero_wavelengths", rng_states="rng_states"),
                            dict(out=((N, K), False))),
    "create_ghost_rays": (lambda c, a, pairs: c.create_ghost_rays(a["samples"], a["rays"], pairs, rng_states=a["rng_states"], out=a["out"]),
                          dict(samples="samples", rays="rays", rng_states="rng_states"), dict(out=((N, 1, 8), False))),
    "create_ghost_rays(wavelengths=)": (lambda c, a, pairs: c.create_ghost_rays(a["samples"], a["rays"], pairs, a["wavelengths"], a["rng_states"],
                                                                                out=a["out"]),
                                        dict(samples="samples", rays="spectral_rays", wavelengths="wavelengths", rng_states="rng_states"),
                                        dict(out=((N, 1, 8), False))),
}
# the calls whose first item may also be a numpy array (it selects their numpy half)
NUMPY_HALF = ("create_rays", "create_rays_hero", "project_points", "trace_back", "pupil_bounds", "splat_points")

# (call, argument) -> the faults the binding used to let through to the library: test_calls_once_accepted_unsoundly_are_refused
ONCE_ACCEPTED = {
    ("create_rays", "out"): ("dtype", "rows", "strided"), ("create_rays(wavelengths=)", "out"): ("dtype", "rows", "strided"),
    ("create_rays", "rng_states"): ("strided", "host", "numpy", "other device"),
    ("create_rays(wavelengths=)", "rng_states"): ("strided", "host", "numpy", "other device"),
    ("ray_differentials", "rng_states"): ("host", "numpy", "other device"),
    ("ray_differentials(wavelengths=)", "rng_states"): ("host", "numpy", "other device"),
    ("create_rays_resident", "samples"): ("host", "numpy", "other device"),
}


def _faults(torch, t, first):
    """fault -> a bad value in place of the well-formed tensor t.  The first item of a call sets n, so its shape fault is a column
    too many, every other argument's a row too many."""
    bad = {"dtype": t.double(),
           "strided": t.repeat_interleave(2, 0)[::2],
           "host": t.cpu(),
           "numpy": t.cpu().numpy()}
    if first:
        bad["columns"] = torch.cat([t, t[:, :1]], 1).contiguous()
    else:
        bad["rows"] = torch.cat([t, t[:1]], 0).contiguous()
    if torch.cuda.device_count() >= 2:
        bad["other device"] = t.to(torch.device("cuda", 1))
    assert bad["strided"].shape == t.shape and not bad["strided"].is_contiguous()
    return bad


def _buffers(setup, results):
    torch = setup.torch
    return {k: torch.full(shape, SENTINEL, dtype=torch.int32, device=setup.dev).view(torch.int32 if integer else torch.float32)
            for k, (shape, integer) in results.items()}


def _bytes(setup, x):
    """a host copy of the bytes of a tensor or an array, in index order"""
    t = x if setup.torch.is_tensor(x) else setup.torch.from_numpy(np.ascontiguousarray(x))
    return t.contiguous().cpu().view(setup.torch.uint8).clone()


def _cases(setup, name, which):
    """(argument, fault, the call's arguments, its result buffers): every fault of every argument that `which`(call, argument, fault)
    picks; the result buffers are filled with the sentinel, a faulty one too"""
    call, reads, results = CALLS[name]
    good = {k: setup.args[v] for k, v in reads.items()}
    first = next(iter(reads))
    for arg in list(reads) + list(results):
        t = good[arg] if arg in reads else _buffers(setup, results)[arg]
        for fault, value in _faults(setup.torch, t, arg == first).items():
            if not which(name, arg, fault):
                continue
            if fault == "numpy" and arg == first and name.split("(")[0].replace("_jacobian", "") in NUMPY_HALF:
                continue   # a numpy item is no fault there
            bufs = _buffers(setup, results)
            if arg in bufs:
                bufs[arg] = value
            yield arg, fault, dict(good, **dict(bufs, **{arg: value})), bufs


def _refused(setup, name, which):
    """the number of faulty calls made, each refused with its exception and each leaving the result buffers as they were"""
    call = CALLS[name][0]
    count = 0
    for arg, fault, a, bufs in _cases(setup, name, which):
        before = {k: _bytes(setup, b) for k, b in bufs.items()}
        with pytest.raises(TypeError if (arg == "wavelengths" and fault == "numpy") else ValueError):
            call(setup.cam, a, setup.pairs)
            pytest.fail("%s accepted %s with the fault: %s" % (name, arg, fault))
        setup.torch.cuda.synchronize(setup.dev)
        for k, b in bufs.items():
            assert setup.torch.equal(_bytes(setup, b), before[k]), (name, arg, fault, k)
        count += 1
    return count


def _once(call, arg, fault):
    return fault in ONCE_ACCEPTED.get((call, arg), ())


@pytest.mark.parametrize("name", sorted(CALLS))
def test_bad_tensor_is_refused_before_any_launch(setup, name):
    """every tensor argument with every fault: the exception, and sentinel-filled result buffers that keep their bits"""
    count = _refused(setup, name, lambda call, arg, fault: not _once(call, arg, fault))
    assert count >= 2 * (len(CALLS[name][1]) + len(CALLS[name][2]))   # (at least two faults of each argument are not in ONCE_ACCEPTED)


def test_calls_once_accepted_unsoundly_are_refused(setup):
    """What the binding used to hand to the library and now refuses with ValueError: a create_rays out["rays"] of the wrong dtype,
    shape or layout; rng_states that are strided, on the host, on another device or no tensor at all; a host, other-device or numpy
    samples array given to create_rays_resident."""
    total = sum(_refused(setup, name, _once) for name in sorted({call for call, _ in ONCE_ACCEPTED}))
    assert total >= 2 * 3 + 2 * 3 + 2 * 2 + 2


def _tensors(res):
    if isinstance(res, dict):
        return [res["rays"]]
    return list(res) if isinstance(res, tuple) else [res]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_caller_buffers_receive_the_bits_of_the_plain_call(setup, name):
    torch = setup.torch
    call, reads, results = CALLS[name]
    good = {k: setup.args[v] for k, v in reads.items()}
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    plain = _tensors(call(setup.cam, dict(good, **{k: None for k in results}), setup.pairs))
    bufs = _buffers(setup, results)
    res = call(setup.cam, dict(good, **bufs), setup.pairs)
    given = _tensors(res)
    torch.cuda.synchronize(setup.dev)
    assert len(plain) == len(given) >= len(results)
    for k, want, got in zip(results, plain, given):
        assert got.data_ptr() == bufs[k].data_ptr() and got.shape == want.shape and got.dtype == want.dtype, (name, k)
    for i, (want, got) in enumerate(zip(plain, given)):
        assert want.data_ptr() != got.data_ptr()
        assert torch.equal(bits(want), bits(got)), (name, i)
        assert not bool((bits(got) == SENTINEL).any()), (name, i)
    if isinstance(res, dict):   # the views of a record dict look into the given buffer
        assert sorted(res) == ["dir", "flags", "origin", "planes", "rays", "weight"]
        r = res["rays"]
        for key, cols in (("origin", slice(0, 3)), ("dir", slice(3, 6)), ("planes", slice(0, 7))):
            assert torch.equal(bits(res[key]), bits(r[..., cols].movedim(-1, 0))), (name, key)
        assert torch.equal(bits(res["weight"]), bits(r[..., 6])) and res["weight"].data_ptr() == r.data_ptr() + 24
        assert res["flags"].dtype == torch.int32 and torch.equal(res["flags"], bits(r[..., 7]))

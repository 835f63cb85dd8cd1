"""The binding's argument rules for the trace-back transmittance methods on the MI355X, in the manner of
tests/test_binding_arguments_gpu.py: every tensor argument of the torch paths of trace_back_transmittance and splat_transmittance is
refused when its dtype, its shape, its layout or its device is wrong, or when it is a numpy array beside torch tensors -- in Python,
before any launch: the sentinel-filled result buffers keep their bits -- and a call given out / screen / flags writes into them the
bits of the same call without them.

One camera (the double Gauss with its dispersion table and films), n = 5 rays / points and m = 1 aim per point: the smallest shapes
at which a mixed-up dimension still shows."""
import numpy as np
import pytest

from zoic_amd import ZoicCamera
from zoic_amd.workloads import ray_rng_states, synthetic_samples

import backward_spectral_ref as bs
import pupil_cases as pc
import traceback_cases as tc
import traceback_throughput_ref as tr
import transmittance_ref as tref

pytestmark = pytest.mark.gpu

N, M = 5, 1
SENTINEL = 0x7FA51234   # a NaN with a payload no kernel writes


class _Setup:
    """the camera and one well-formed value for every tensor argument (device tensors, read only)"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        p = pc.params_of("C3")
        cam = self.cam = tc.update(ZoicCamera(device=0), p)
        bs.set_dispersion(cam, pc.CAMERAS["C3"][0])
        tr.coat(cam, tref.films_where_media_differ(cam.dispersion()))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
        a = dict(samples=up(synthetic_samples(N, 64, 36, 1, seed=3)), rng_states=up(ray_rng_states(N, seed=3).view(np.int32)),
                 wavelengths=up(np.array([450.0, 500.0, 550.0, 600.0, 650.0], np.float32)), points=up(pc.points(p)[:N]),
                 u=up(np.random.default_rng(5).random((N, M, 2)).astype(np.float32)))
        a["rays"] = cam.create_rays(a["samples"], rng_states=a["rng_states"])["rays"]
        a["spectral_rays"] = cam.create_rays(a["samples"], rng_states=a["rng_states"], wavelengths=a["wavelengths"])["rays"]
        a["bounds"] = cam.pupil_bounds(a["points"])
        torch.cuda.synchronize(self.dev)
        assert (a["rays"][:, 6] > 0).any() and (a["bounds"].view(torch.int32)[:, 8] > 0).any()
        self.args = a


@pytest.fixture(scope="module")
def setup(gpu):
    s = _Setup()
    yield s
    s.cam.close()


# name -> (call(cam, a) with a the dict of its tensor arguments (a result buffer may be None),
#          the arguments read: name in the call -> name in the setup; the first one is the item that sets n,
#          the result buffers: name -> (shape, integer?))
CALLS = {
    "trace_back_transmittance": (lambda c, a: c.trace_back_transmittance(a["rays"], out=a["out"], screen=a["screen"], flags=a["flags"]),
                                 dict(rays="rays"), dict(out=((N,), False), screen=((N, 2), False), flags=((N,), True))),
    "trace_back_transmittance(wavelengths=)": (
        lambda c, a: c.trace_back_transmittance(None if a["rays"] is None else dict(rays=a["rays"]), a["wavelengths"], a["out"], a["screen"],
                                                a["flags"]),
        dict(rays="spectral_rays", wavelengths="wavelengths"), dict(out=((N,), False), screen=((N, 2), False), flags=((N,), True))),
    "splat_transmittance": (lambda c, a: c.splat_transmittance(a["points"], a["bounds"], a["u"], out=a["out"]),
                            dict(points="points", bounds="bounds", u="u"), dict(out=((N, M), False))),
    "splat_transmittance(wavelengths=)": (lambda c, a: c.splat_transmittance(a["points"], a["bounds"], a["u"], a["wavelengths"], out=a["out"]),
                                          dict(points="points", bounds="bounds", u="u", wavelengths="wavelengths"), dict(out=((N, M), False))),
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


@pytest.mark.parametrize("name", sorted(CALLS))
def test_bad_tensor_is_refused_before_any_launch(setup, name):
    """every tensor argument with every fault (a numpy array in place of the items too: the result buffers are torch tensors, which
    the numpy half refuses): the exception, and sentinel-filled result buffers that keep their bits"""
    call, reads, results = CALLS[name]
    good = {k: setup.args[v] for k, v in reads.items()}
    first = next(iter(reads))
    count = 0
    for arg in list(reads) + list(results):
        t = good[arg] if arg in reads else _buffers(setup, results)[arg]
        for fault, value in _faults(setup.torch, t, arg == first).items():
            bufs = _buffers(setup, results)
            if arg in bufs:
                bufs[arg] = value
            before = {k: _bytes(setup, b) for k, b in bufs.items()}
            with pytest.raises(TypeError if (arg == "wavelengths" and fault == "numpy") else ValueError):
                call(setup.cam, dict(good, **dict(bufs, **{arg: value})))
                pytest.fail("%s accepted %s with the fault: %s" % (name, arg, fault))
            setup.torch.cuda.synchronize(setup.dev)
            for k, b in bufs.items():
                assert setup.torch.equal(_bytes(setup, b), before[k]), (name, arg, fault, k)
            count += 1
    assert count >= 5 * (len(reads) + len(results))


@pytest.mark.parametrize("name", sorted(CALLS))
def test_caller_buffers_receive_the_bits_of_the_plain_call(setup, name):
    torch = setup.torch
    call, reads, results = CALLS[name]
    good = {k: setup.args[v] for k, v in reads.items()}
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    tensors = lambda res: list(res) if isinstance(res, tuple) else [res]  # noqa: E731
    plain = tensors(call(setup.cam, dict(good, **{k: None for k in results})))
    bufs = _buffers(setup, results)
    given = tensors(call(setup.cam, dict(good, **bufs)))
    torch.cuda.synchronize(setup.dev)
    assert len(plain) == len(given) == len(results)
    for k, want, got in zip(results, plain, given):
        assert got.data_ptr() == bufs[k].data_ptr() != want.data_ptr() and got.shape == want.shape and got.dtype == want.dtype, (name, k)
        assert torch.equal(bits(want), bits(got)) and not bool((bits(got) == SENTINEL).any()), (name, k)
    assert bool((plain[0] > 0).any())

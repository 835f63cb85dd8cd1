"""The one-record-per-lane passes behind a thin-lens camera, past one grid's worth: n = 2048 x 256 + 65 rows, the first size at which
a grid-stride loop takes a second turn and that turn ends in a partial wave.  Four calls on camera C1 (THINLENS with depth of field, no
vignetting): transmittance at k = 1, ghost rays at p = 1, spectral rays and hero rays at k = 2.

Every expected value comes from the calls' documented contract and from zoic_create_rays_device, whose records are compared with the
CPU oracle here first (all of them are live and counted as successes: the oracle says so).  Wavelengths cycle through valid values,
one below 360 nm and a NaN, with a period that is odd: every kind lands in the second turn."""
import numpy as np
import pytest

from zoic_amd.workloads import ray_rng_states

import ghost_ref as gref
from device_cases import BIG, bits as _words, bits_f32 as _bits, camera as _camera, delta as _delta, oracle as _oracle, params as _params, samples as _samples
from spectral_ref import LAMBDA_D

pytestmark = pytest.mark.gpu

FIRST_TURN = 2048 * 256
CYCLE = np.array([450.0, 550.0, 359.0, 650.0, LAMBDA_D, np.nan, 830.0], np.float32)   # 359: below the range
REJECTED = 0x80


def _valid(lam):
    return (lam >= 360.0) & (lam <= 830.0)      # false for NaN


@pytest.fixture(scope="module")
def thin(gpu, oracle_lib):
    """(camera, samples on the device, wavelengths (n,), the plain call's records (n, 8) as words, its counters) -- read-only"""
    import torch
    assert BIG == FIRST_TURN + 65
    p = _params("C1")
    cam = _camera(p)
    s = _samples(BIG, seed=19)
    ts = torch.from_numpy(s).cuda()
    rays, counted = _delta(cam, lambda: cam.create_rays(ts)["rays"].clone())
    plain = _words(rays.cpu().numpy())
    ref = _oracle(oracle_lib, p).create_rays(s, rng_states=ray_rng_states(BIG, seed=1))
    assert np.array_equal(plain[:, 0:6], _bits(ref["planes"][0:6].T)) and np.array_equal(plain[:, 6], _bits(ref["weight"]))
    assert np.array_equal(plain[:, 7], ref["flags"].astype(np.uint32))
    assert (ref["weight"] != 0).all()                                    # live throughout: what the four tests rely on
    assert counted == dict(succesRays=BIG, vignettedRays=0, totalInternalReflection=0)
    lam = np.resize(CYCLE, BIG)
    assert _valid(lam[FIRST_TURN:]).any() and (~_valid(lam[FIRST_TURN:])).sum() >= 2
    plain.setflags(write=False)
    lam.setflags(write=False)
    yield cam, ts, rays, lam, plain
    cam.close()


def test_transmittance_of_a_thin_lens(thin):
    """exactly 1.0 where the record has weight and the wavelength is valid, +0.0 elsewhere"""
    import torch
    cam, ts, rays, lam, plain = thin
    got = cam.transmittance(ts, rays, wavelengths=torch.from_numpy(np.array(lam)).cuda()).cpu().numpy().reshape(-1)
    want = ((plain[:, 6] != 0) & _valid(lam)).astype(np.float32)
    assert got.shape == (BIG,) and np.array_equal(_bits(got), _bits(want))
    assert (want[FIRST_TURN:] == 1.0).any() and (want[FIRST_TURN:] == 0.0).any()


def test_ghost_rays_of_a_thin_lens(thin):
    """a lens without interfaces has no ghosts: every record is the dead record of reason MODEL, all eight words"""
    import torch
    cam, ts, rays, lam, plain = thin
    dead = np.zeros(8, np.uint32)
    dead[7] = gref.flag_word(gref.MODEL, 0, 0)
    for w in (None, torch.from_numpy(np.array(lam)).cuda()):
        got = _words(cam.create_ghost_rays(ts, rays, np.array([(3, 1)]), wavelengths=w).cpu().numpy()).reshape(-1, 8)
        assert got.shape == (BIG, 8) and (got == dead).all()
    assert (plain[FIRST_TURN:, 6] != 0).any()                            # the main records of the second turn are live


def test_spectral_rays_of_a_thin_lens(thin):
    """rows with a valid wavelength are the plain call's, the others the rejected record; the counters are the plain call's minus the
    rejected rows (every plain row is a success)"""
    import torch
    cam, ts, _, lam, plain = thin
    rays, counted = _delta(cam, lambda: cam.create_rays(ts, wavelengths=torch.from_numpy(np.array(lam)).cuda())["rays"])
    got = _words(rays.cpu().numpy())
    ok = _valid(lam)
    assert np.array_equal(got[ok], plain[ok])
    assert (got[~ok, 0:7] == 0).all() and (got[~ok, 7] == REJECTED).all()
    assert counted == dict(succesRays=int(ok.sum()), vignettedRays=0, totalInternalReflection=0)
    assert (got[FIRST_TURN:][ok[FIRST_TURN:], 6] != 0).any() and (~ok[FIRST_TURN:]).any()


def test_hero_rays_of_a_thin_lens(thin):
    """row (i, j) is the plain record where the hero and column j are valid, the rejected record otherwise; a rejected hero's count is
    taken back"""
    import torch
    cam, ts, _, lam, plain = thin
    lam2 = np.stack([lam, np.roll(lam, 3)], 1)                           # (hero, companion): valid / invalid in all four combinations
    rays, counted = _delta(cam, lambda: cam.create_rays_hero(ts, torch.from_numpy(np.ascontiguousarray(lam2)).cuda())["rays"])
    got = _words(rays.cpu().numpy())
    assert got.shape == (BIG, 2, 8)
    hero = _valid(lam2[:, 0])
    for j in range(2):
        ok = hero & _valid(lam2[:, j])
        assert np.array_equal(got[ok, j], plain[ok])
        assert (got[~ok, j, 0:7] == 0).all() and (got[~ok, j, 7] == REJECTED).all()
        assert (got[FIRST_TURN:, j][ok[FIRST_TURN:], 6] != 0).any() and (~ok[FIRST_TURN:]).any()
    assert (hero & ~_valid(lam2[:, 1])).any() and (~hero & _valid(lam2[:, 1])).any()
    assert counted == dict(succesRays=int(hero.sum()), vignettedRays=0, totalInternalReflection=0)

"""Rays at a wavelength per ray on the MI355X (zoic_create_rays_spectral_device): the d-line reproduces zoic_create_rays_device bit for
bit, other wavelengths reproduce the oracle run on the per-wavelength index table, FAST agrees with STRICT, blue focuses closer than
red, and rejected wavelengths, determinism, launch splits, the thin lens and the error codes behave as the header states."""
import numpy as np
import pytest

from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import ray_rng_states

from fuzz_cameras import _oracle_spectral
from device_cases import bits_f32 as _bits, camera as _camera, delta as _delta, params as _params, samples as _samples
from spectral_ref import BAD, LAMBDA_D, SINGLET, WAVES

pytestmark = pytest.mark.gpu

def _records_equal(a, b):
    assert np.array_equal(a["flags"], b["flags"])
    assert np.array_equal(_bits(a["planes"]), _bits(b["planes"]))


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_d_line_is_the_plain_call(cfg):
    """STRICT at 587.5618 nm: records (all 8 words) and counters bit-identical to zoic_create_rays_device"""
    n = 1 << 17
    p = _params(cfg)
    cam = _camera(p)
    s = _samples(n)
    plain, cp = _delta(cam, lambda: cam.create_rays(s, ray_index_base=7))
    spec, cs = _delta(cam, lambda: cam.create_rays(s, ray_index_base=7, wavelengths=np.full(n, LAMBDA_D, np.float32)))
    _records_equal(spec, plain)
    assert cs == cp
    cam.close()


def test_four_column_lens_ignores_the_wavelength():
    """DOUBLE_GAUSS ships no V-numbers: without an override every valid wavelength gives the d-line records"""
    n = 1 << 15
    cam = _camera(_params("C3"))
    assert not cam.dispersion()["cauchy_b"].any()
    s = _samples(n)
    plain = cam.create_rays(s)
    lam = np.random.RandomState(3).uniform(360, 830, n).astype(np.float32)
    lam[:4] = [360.0, 830.0, 486.1327, 656.2725]
    _records_equal(cam.create_rays(s, wavelengths=lam), plain)
    cam.close()


PARITY = [
    ("C2", {}, None),
    ("C5", {}, None),
    ("C2", dict(useImage=True), None),
    ("C2", dict(useImage=True, kolbSamplingLUT=False), None),
    ("C3", {}, "synthetic"),
]


@pytest.mark.parametrize("cfg,over,abbe", PARITY, ids=["C2", "C5", "tessar-bokeh-lut", "tessar-bokeh-nolut", "dgauss-override"])
def test_strict_matches_oracle(oracle_lib, cfg, over, abbe):
    n = 1 << 15
    p = _params(cfg, **over)
    V = None
    if abbe:
        count = ZoicCamera(device=-1).update(**dict(p, useImage=False)).info()["lensCount"]
        V = np.linspace(35.0, 64.0, count).astype(np.float32)
    cam = _camera(p, abbe=V)
    disp = cam.dispersion()
    assert disp["cauchy_b"].any()
    s = _samples(n, seed=11)
    lam = np.resize(WAVES, n)                     # eight wavelengths interleaved ray by ray, one call
    states = ray_rng_states(n, seed=2)
    got, cg = _delta(cam, lambda: cam.create_rays(s, rng_states=states, wavelengths=lam))
    ref, cr = _oracle_spectral(oracle_lib, p, disp, s, lam, states)
    assert np.array_equal(got["flags"], ref["flags"])
    g, r = got["planes"], ref["planes"]
    same = (_bits(g) == _bits(r)) | (np.isnan(g) & np.isnan(r))
    assert same.all(), int((~same.all(0)).sum())
    assert cg == cr
    # not the d-line's rays: the wavelengths changed something
    plain = cam.create_rays(s, rng_states=states)
    assert not np.array_equal(_bits(plain["planes"]), _bits(g))
    cam.close()


@pytest.mark.parametrize("cfg,abbe", [("C2", None), ("C5", None), ("C3", 50.0)])
def test_fast_agrees_with_strict(cfg, abbe):
    n = 1 << 18
    p = _params(cfg)
    V = None
    if abbe:
        V = np.full(ZoicCamera(device=-1).update(**dict(p, useImage=False)).info()["lensCount"], abbe, np.float32)
    strict = _camera(p, PRECISION_STRICT, V)
    fast = _camera(p, PRECISION_FAST, V)
    assert not fast.info()["fastRunsStrict"]
    s = _samples(n, seed=21)
    lam = np.random.RandomState(4).uniform(400, 700, n).astype(np.float32)
    a = strict.create_rays(s, wavelengths=lam)
    b = fast.create_rays(s, wavelengths=lam)
    differ = (a["flags"] != b["flags"]) | (a["weight"] != b["weight"])
    assert differ.mean() <= 5e-5, differ.sum()
    live = ~differ & (a["weight"] != 0) & np.isfinite(a["dir"]).all(0)
    err = (a["dir"][:, live].astype(np.float64) - b["dir"][:, live]) ** 2
    assert np.sqrt(err.sum(0).mean()) < 1e-5
    assert not np.array_equal(_bits(a["planes"][:, live]), _bits(b["planes"][:, live]))   # FAST is not the STRICT kernel
    strict.close(); fast.close()


def test_fast_runs_strict_camera_gives_strict_bits():
    p = _params("C2", focalLength=-10.0)          # negative focal-length ratio: outside the FAST modes' domain
    strict = _camera(p, PRECISION_STRICT)
    fast = _camera(p, PRECISION_FAST)
    assert fast.info()["fastRunsStrict"]
    n = 1 << 15
    s = _samples(n, seed=8)
    lam = np.random.RandomState(5).uniform(400, 700, n).astype(np.float32)
    _records_equal(fast.create_rays(s, wavelengths=lam), strict.create_rays(s, wavelengths=lam))
    strict.close(); fast.close()


def test_blue_focuses_closer_than_red():
    """physics without the oracle: an on-axis sensor point through a positive singlet; the rays' crossing of the axis in object space"""
    cam = ZoicCamera(device=0)
    cam.set_lens_text(SINGLET)
    cam.update(**_params("C2", focalLength=5.0, fStop=4.0, kolbSamplingLUT=False, focalDistance=100.0))
    n = 1 << 14
    rs = np.random.RandomState(9)
    s = np.ascontiguousarray(np.stack([np.zeros(n), np.zeros(n), rs.uniform(0, 1, n), rs.uniform(0, 1, n)], 1), np.float32)
    cross = {}
    for w in (450.0, LAMBDA_D, 650.0):
        r = cam.create_rays(s, wavelengths=np.full(n, w, np.float32))
        live = r["weight"] != 0
        O, D = r["origin"][:, live].astype(np.float64), r["dir"][:, live].astype(np.float64)
        rho2 = D[0] ** 2 + D[1] ** 2
        ok = rho2 > 1e-12
        t = -(O[0, ok] * D[0, ok] + O[1, ok] * D[1, ok]) / rho2[ok]
        assert ok.sum() > 200, (w, float(live.mean()), int(ok.sum()))
        cross[w] = float(np.median(t))
    assert cross[450.0] < cross[LAMBDA_D] < cross[650.0], cross
    cam.close()


@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_rejected_wavelengths(cfg):
    n = 4096
    cam = _camera(_params(cfg, **({"opticalVignettingDistance": 5.0} if cfg == "C1" else {})))
    s = _samples(n, seed=13)
    lam = np.random.RandomState(6).uniform(360, 830, n).astype(np.float32)
    rows = np.arange(len(BAD)) * 97 + 5
    good = lam.copy()
    good[rows] = LAMBDA_D
    ref, cref = _delta(cam, lambda: cam.create_rays(s, wavelengths=good))
    lam[rows] = BAD
    got, cgot = _delta(cam, lambda: cam.create_rays(s, wavelengths=lam))
    assert (got["flags"][rows] == 0x80).all()
    assert (_bits(got["planes"][:, rows]) == 0).all()
    keep = np.ones(n, bool)
    keep[rows] = False
    assert np.array_equal(got["flags"][keep], ref["flags"][keep])
    assert np.array_equal(_bits(got["planes"][:, keep]), _bits(ref["planes"][:, keep]))
    # the rejected rows count nowhere: a batch of just those rows at the d-line (the others rejected) adds up to the difference
    only = np.where(keep, np.float32(np.nan), np.float32(LAMBDA_D)).astype(np.float32)
    _, conly = _delta(cam, lambda: cam.create_rays(s, wavelengths=only))
    assert {k: cgot[k] + conly[k] for k in cgot} == cref
    cam.close()


def test_deterministic_and_split_launches():
    import torch
    n = 1 << 16
    cam = _camera(_params("C5"), PRECISION_FAST)
    s = torch.from_numpy(_samples(n, seed=17)).cuda()
    lam = torch.from_numpy(np.random.RandomState(7).uniform(400, 700, n).astype(np.float32)).cuda()
    whole = cam.create_rays(s, wavelengths=lam, ray_index_base=1000)["rays"].clone()
    again = cam.create_rays(s, wavelengths=lam, ray_index_base=1000)["rays"].clone()
    parts = torch.empty_like(whole)
    cut = [0, 5000, 40000, n]
    for a, b in zip(cut[:-1], cut[1:]):
        parts[a:b] = cam.create_rays(s[a:b].contiguous(), wavelengths=lam[a:b].contiguous(), ray_index_base=1000 + a)["rays"]
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
    cam.close()


def test_thin_lens_ignores_the_wavelength():
    n = 1 << 14
    cam = _camera(_params("C1", opticalVignettingDistance=5.0))
    s = _samples(n, seed=19)
    plain, cp = _delta(cam, lambda: cam.create_rays(s))
    lam = np.random.RandomState(8).uniform(360, 830, n).astype(np.float32)
    spec, cs = _delta(cam, lambda: cam.create_rays(s, wavelengths=lam))
    _records_equal(spec, plain)
    assert cs == cp
    cam.close()


def test_error_codes():
    import torch
    from zoic_amd import _capi
    L = _capi.load()
    cam = ZoicCamera(device=0)
    s = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    lam = torch.full((65,), LAMBDA_D, dtype=torch.float32, device="cuda")
    out = torch.empty((64, 8), dtype=torch.float32, device="cuda")
    call = lambda n, w: L.zoic_create_rays_spectral_device(cam._h, n, s.data_ptr(), w, None, 0, out.data_ptr(), None)
    assert call(64, lam.data_ptr()) == _capi.STATUS_NAMES.index("ZOIC_ERR_NOT_UPDATED")
    cam.update(**_params("C2"))
    assert call(64, None) == _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
    assert call(64, lam.data_ptr() + 2) == _capi.STATUS_NAMES.index("ZOIC_ERR_INVALID_ARGUMENT")
    assert call(0, lam.data_ptr()) == 0
    assert call(64, lam.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        cam.create_rays(s, wavelengths=np.full(64, LAMBDA_D, np.float32))
    cam.close()

"""What the device tests of the batch calls share: parameters, a camera on device 0, its oracle, random screen samples, counter deltas,
ray records from (origin, dir), and the two bit views of an array.  A helper, not a test."""
import numpy as np

from zoic_amd import PRECISION_STRICT, ZoicCamera
from zoic_amd.workloads import camera_params, hexagon_bokeh

BIG = 2048 * 256 + 65      # the first size at which a grid-stride loop takes a second turn and that turn ends in a partial wave


def params(cfg, **over):
    p = camera_params(cfg)
    p.update(over)
    return p


def camera(p, precision=PRECISION_STRICT, abbe=None):
    cam = ZoicCamera(device=0)
    if p.get("useImage"):
        cam.set_bokeh_image(hexagon_bokeh())
    cam.set_precision(precision)
    if abbe is not None:
        cam.set_abbe_numbers(abbe)
    cam.update(**p)
    return cam


def oracle(oracle_lib, p):
    oc = oracle_lib.OracleCamera()
    if p.get("useImage"):
        oc.set_bokeh_image(hexagon_bokeh())
    oc.update(**p)
    return oc


def samples(n, aspect=16 / 9, seed=5):
    """random screen samples over the whole frame (a frame's first rays in lattice order would all sit in one corner)"""
    rs = np.random.RandomState(seed)
    s = np.stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n) / aspect, rs.uniform(0, 1, n), rs.uniform(0, 1, n)], 1)
    return np.ascontiguousarray(s, np.float32)


def spectral_run(cam, s_np, lam_np, chromatic=True, states=None, base=0, **kw):
    """records and differentials of one spectral batch: (rays (n,8), diffs (n,12), chroma (n,6) or None) as numpy"""
    import torch
    s = torch.from_numpy(s_np).cuda()
    lam = torch.from_numpy(lam_np).cuda()
    st = None if states is None else torch.from_numpy(states.view(np.int32)).cuda()
    rays = cam.create_rays(s, wavelengths=lam, rng_states=st, ray_index_base=base)["rays"]
    r = cam.ray_differentials(s, rays, rng_states=st, ray_index_base=base, wavelengths=lam, chromatic=chromatic, **kw)
    torch.cuda.synchronize()
    d, c = r if chromatic else (r, None)
    return rays.cpu().numpy(), d.cpu().numpy(), None if c is None else c.cpu().numpy()


def delta(cam, fn):
    before = cam.counters()
    r = fn()
    after = cam.counters()
    return r, {k: after[k] - before[k] for k in after}


def records(o, d):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6] = 1.0
    return r


def bits(a):
    """the array's own 32-bit words (a uint32 flag word stays what it is)"""
    return np.ascontiguousarray(a).view(np.uint32)


def bits_f32(a):
    """the words of the array cast to float32 first"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

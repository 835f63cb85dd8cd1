"""Host-side mirror of zoic's Arnold camera node over the C-ABI (libzoic_amd.so).

    cam = ZoicCamera(device=0)                       # node_initialize   zoic.cpp:1565-1572
    cam.update(lensModel=RAYTRACED, lensDataPath=..) # node_update       zoic.cpp:1575-1720 (14 parameters, same names)
    rays = cam.create_rays(samples)                  # camera_create_ray zoic.cpp:1752-1990, batched
    cam.close()                                      # node_finish       zoic.cpp:1723-1749

Parameter names, defaults and error behaviour follow node_parameters (zoic.cpp:1547-1562).  Errors the reference
reports with AiMsgError + AiRenderAbort() surface as ZoicError with the same message text.

This module only marshals pointers; all rays come from the HIP kernels.  torch tensors (device memory) and numpy
arrays (host memory) are both accepted.
"""
import ctypes as C
import weakref
import os

import numpy as np

from . import _capi
from ._capi import PRECISION_FAST, PRECISION_FAST_UNCHECKED, PRECISION_STRICT, RAYTRACED, THINLENS  # noqa: F401

LENS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lenses")

# node_parameters, zoic.cpp:1547-1562
DEFAULTS = dict(sensorWidth=3.6, sensorHeight=2.4, focalLength=2.0, fStop=4.0, focalDistance=100.0, useImage=False,
                bokehPath="", lensModel=RAYTRACED, lensDataPath="", kolbSamplingLUT=True, useDof=True,
                opticalVignettingDistance=0.0, opticalVignettingRadius=1.0, exposureControl=0.0)
_STR = ("bokehPath", "lensDataPath")
_INT = ("useImage", "lensModel", "kolbSamplingLUT", "useDof")

FLAG_RETRIED = 1
FLAG_LUT_MISS = 64
HERO_MAX_WAVELENGTHS = _capi.HERO_MAX_WAVELENGTHS   # zoic_create_rays_hero_device: wavelengths per sample
RAY_COMPANION_LOST = _capi.RAY_COMPANION_LOST       # flag bit 8 of a companion record: lost at the hero's lens point


def lens_path(name):
    """Path of a bundled lens prescription (zoic_amd/lenses/*.dat)."""
    p = os.path.join(LENS_DIR, name)
    if not os.path.exists(p):
        raise FileNotFoundError(p)
    return p


class ZoicError(RuntimeError):
    def __init__(self, status, detail):
        name = _capi.STATUS_NAMES[status] if 0 <= status < len(_capi.STATUS_NAMES) else str(status)
        super().__init__("%s: %s" % (name, detail))
        self.status = status
        self.status_name = name


# a ghost pair as the C-ABI packs it: a | b << 8 (ZOIC_GHOST_PAIR)
_GHOST_INDEX_BITS = 8
_GHOST_INDEX_MASK = (1 << _GHOST_INDEX_BITS) - 1


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _records(rays):
    """the record buffer of a `rays` argument: the dict of a create_rays call stands for its "rays" entry"""
    return rays["rays"] if isinstance(rays, dict) else rays


def _ray_views(rays):
    """the strided views a forward call on device tensors returns beside its (n,8) or (n,k,8) float32 record tensor"""
    import torch
    planes = rays[..., 0:7].movedim(-1, 0)
    return dict(origin=planes[0:3], dir=planes[3:6], weight=planes[6], planes=planes, flags=rays[..., 7].view(torch.int32))


def _host_records(rays):
    """the structured zoic_ray records, shape (n,) or (n,k), of a record tensor whose stream has been waited for"""
    a = np.ascontiguousarray(rays.cpu().numpy())
    return a.view(_capi.RAY_DTYPE).reshape(a.shape[:-1])


# what the numpy half of a batch call makes of its further arrays before they go to the device (n: the number of items)
def _f32(a, n):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f32_flat(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _hero_wavelengths(a, n):
    w = np.ascontiguousarray(a, dtype=np.float32)
    if w.ndim != 2 or w.shape[0] != n:
        raise ValueError("wavelengths must be (n, k)")
    return w


def _rng_words(a, n):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _bounds_floats(a, n):
    return np.ascontiguousarray(pupil_bounds_records(a)).view(np.float32).reshape(-1, 12)


def rays_to_dict(rays):
    """(n,) zoic_ray records -> convenience views (planes are copies: ox oy oz dx dy dz weight)."""
    planes = np.stack([rays[k] for k in ("ox", "oy", "oz", "dx", "dy", "dz", "weight")]).astype(np.float32, copy=False)
    flags = rays["flags"].astype(np.uint8)
    return dict(rays=rays, planes=planes, origin=planes[0:3], dir=planes[3:6], weight=planes[6], flags=flags,
                tries=((flags >> 1) & 31).astype(np.int32))


def hero_rays_to_dict(rays):
    """(n, k) zoic_ray records of create_rays_hero -> the views of rays_to_dict with the (n, k) axes last; flags keep all their bits
    (uint32: bit 8 is RAY_COMPANION_LOST)."""
    planes = np.stack([rays[k] for k in ("ox", "oy", "oz", "dx", "dy", "dz", "weight")]).astype(np.float32, copy=False)
    flags = rays["flags"].astype(np.uint32)
    return dict(rays=rays, planes=planes, origin=planes[0:3], dir=planes[3:6], weight=planes[6], flags=flags,
                tries=((flags >> 1) & 31).astype(np.int32))


def solid_angle_measure(jac, dirs, basis=None):
    """dPs/d(omega) of traced-back rays: det(J_d |d| [e1 e2]), signed, shape (n,) -- what a splatter divides by.

    jac: (n,2,6) Jacobians of ZoicCamera.trace_back_jacobian (or one (2,6)); dirs: the (n,3) directions they were taken at, at the
    length they were given (J_d is the derivative with respect to dir as given, so a step d(omega) of the unit direction is a step
    |d| d(omega) of dir).  numpy in, numpy out (float64); torch in, torch out (the inputs' dtype and device).  No kernel.

    (e1, e2) is any right-handed orthonormal basis of the plane across d (e1 x e2 = d / |d|).  The result does not depend on the
    choice of basis: with a, b the two rows of J_d, det([a; b] [e1 e2]) = (a x b) . (e1 x e2) = (a x b) . d / |d|, which is what is
    evaluated when basis is None; another right-handed basis is the first turned about d, a factor of determinant 1.
    basis: optional (e1, e2), each (n,3), to evaluate the determinant with that basis literally."""
    if _is_torch(jac):
        import torch
        J = jac.reshape(-1, 2, 6)[:, :, 3:6]
        d = dirs.reshape(-1, 3).to(J.dtype)
        if basis is None:
            return (torch.linalg.cross(J[:, 0], J[:, 1]) * d).sum(1) * torch.linalg.norm(d, dim=1)
        E = torch.stack([basis[0].reshape(-1, 3).to(J.dtype), basis[1].reshape(-1, 3).to(J.dtype)], 2)
        return torch.linalg.det(J @ E) * (d * d).sum(1)
    J = np.asarray(jac, np.float64).reshape(-1, 2, 6)[:, :, 3:6]
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    if basis is None:
        return (np.cross(J[:, 0], J[:, 1]) * d).sum(1) * np.linalg.norm(d, axis=1)
    E = np.stack([np.asarray(basis[0], np.float64).reshape(-1, 3), np.asarray(basis[1], np.float64).reshape(-1, 3)], 2)
    A = J @ E
    return (A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]) * (d * d).sum(1)


def pupil_bounds_records(bounds):
    """the (n,) structured array (_capi.PUPIL_BOUNDS_DTYPE) of the (n,12) float32 records ZoicCamera.pupil_bounds returns for device
    points (a tensor is copied to the host; the caller has waited for its stream)"""
    if _is_torch(bounds):
        bounds = bounds.cpu().numpy()
    a = np.ascontiguousarray(bounds)
    if a.dtype == np.dtype(_capi.PUPIL_BOUNDS_DTYPE):
        return a.reshape(-1)
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 12).view(_capi.PUPIL_BOUNDS_DTYPE).reshape(-1)


def splat_records(splats):
    """the structured array (_capi.SPLAT_DTYPE: sx, sy, ax, ay, area, angle, flags, reserved) of the (n,m,8) float32 records
    ZoicCamera.splat_points returns, shape (n,m) (a tensor is copied to the host; the caller has waited for its stream)"""
    if _is_torch(splats):
        splats = splats.cpu().numpy()
    a = np.ascontiguousarray(splats)
    if a.dtype == np.dtype(_capi.SPLAT_DTYPE):
        return a
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim < 1 or a.shape[-1] != 8:
        raise ValueError("splats must be (..., 8) float32 records")
    return a.view(_capi.SPLAT_DTYPE).reshape(a.shape[:-1])


def pupil_rays(points, bounds, u, aim_z=0.0):
    """Rays from scene points towards their pupil boxes: (origins (n,3), dirs (n,3), pdf_area (n,)) float32, the rays to hand to
    ZoicCamera.trace_back_jacobian.

    points: (n,3) scene points; bounds: their pupil-bounds records (the structured array, or the (n,12) float32 records);
    u: (n,2) numbers in [0,1)^2, the caller's own (this function draws nothing); aim_z: the z of the aims' plane
    (ZoicCamera.pupil_square()[0]).  Aim i = (aim.min + u_i (aim.max - aim.min), aim_z): uniform in the point's `aim` box;
    origins = points, dirs = points - aims (into the scene, as the trace-back wants), pdf_area = 1 / the box's area (per cm^2 on
    the aims' plane), and 0 for a point with count = 0 (its dir aims at the axis and is refused as every other ray from there).

    Pure host code, numpy only.  The box holds the lattice's passing aims, not exactly the pupil: a ray drawn in it is still traced
    back and may be refused, and how the traced ones are weighted -- by pdf_area, the Jacobian, a filter -- is the caller's."""
    b = pupil_bounds_records(bounds)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
    if not (len(b) == len(p) == len(u)):
        raise ValueError("points, bounds and u must have one row per point")
    lo, hi = b["aim"][:, 0:2], b["aim"][:, 2:4]
    aims = np.empty_like(p)
    aims[:, 0:2] = np.clip(lo + u * (hi - lo), lo, hi)
    aims[:, 2] = np.float32(aim_z)
    area = (hi[:, 0] - lo[:, 0]).astype(np.float64) * (hi[:, 1] - lo[:, 1]).astype(np.float64)
    some = (b["count"] > 0) & (area > 0)
    pdf = np.zeros(len(p), np.float32)
    pdf[some] = (1.0 / area[some]).astype(np.float32)
    return p, p - aims, pdf


class PinnedArray:
    """A numpy array over page-locked host memory (zoic_host_alloc): buffers of this kind let create_rays' host path
    run as an asynchronous two-stream pipeline.  Keep the object alive as long as the array is used."""

    def __init__(self, shape, dtype):
        self._lib = _capi.load()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        st = self._lib.zoic_host_alloc(max(n, 1), C.byref(p))
        if st != 0:
            raise ZoicError(st, (self._lib.zoic_last_error_string() or b"").decode(errors="replace"))
        self._p = p
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.zoic_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ZoicTile:
    """A render thread's bucket of samples (zoic_tile_*): page-locked AtCameraInput / AtCameraOutput arrays the camera's
    RESIDENT kernel reads and writes in place -- no launch, no stream, no copy.

        tile = cam.tile(capacity=64 * 64 * 16, tid=3)
        tile.inputs[:n, (0, 1, 4, 5)] = samples       # (capacity, 7) float32 view: sx sy dsx dsy lensx lensy relative_time
        tile.submit(n, ray_index_base)                # returns at once
        tile.wait()                                   # tile.outputs[:n] -- (capacity, 21) float32 AtCameraOutput rows -- are complete
    Row i equals zoic_create_rays_arnold's row for the same sample and ray index, bit for bit."""

    def __init__(self, cam, capacity, tid=0):
        self._cam = cam
        self._lib = cam._lib
        h = C.c_void_p()
        self._h = None
        cam._check(self._lib.zoic_tile_create(cam._h, int(capacity), int(tid) & 0xFFFF, C.byref(h)))
        self._h = h
        cam._tiles.add(self)   # weak: ZoicCamera.close() closes the tiles still alive first (their views point into memory the camera's end frees)
        self.capacity = int(self._lib.zoic_tile_capacity(h))
        self.tid = int(tid)
        pin = C.cast(self._lib.zoic_tile_inputs(h), C.c_void_p).value
        pout = C.cast(self._lib.zoic_tile_outputs(h), C.c_void_p).value
        self.inputs = np.frombuffer((C.c_char * (self.capacity * 28)).from_address(pin), dtype=np.float32).reshape(self.capacity, 7)
        self.outputs = np.frombuffer((C.c_char * (self.capacity * 84)).from_address(pout), dtype=np.float32).reshape(self.capacity, 21)
        # the same memory as (capacity, 4) float32 samples (sx, sy, lensx, lensy): what the kernel reads after set_inputs(1)
        self.samples = np.frombuffer((C.c_char * (self.capacity * 16)).from_address(pin), dtype=np.float32).reshape(self.capacity, 4)
        # the same memory as (capacity, 8) float32 zoic_ray records: what the kernel writes after set_rows(1)
        self.rays = np.frombuffer((C.c_char * (self.capacity * 32)).from_address(pout), dtype=np.float32).reshape(self.capacity, 8)

    def set_rows(self, rows):
        """0: AtCameraOutput rows in `outputs` (the default); 1: zoic_ray records in `rays` (32 instead of 84 bytes a ray across PCIe)."""
        self._cam._check(self._lib.zoic_tile_set_rows(self._h, int(rows)))

    def set_inputs(self, inputs):
        """0: AtCameraInput rows in `inputs` (the default); 1: (sx, sy, lensx, lensy) in `samples` (16 instead of 28 bytes a sample)."""
        self._cam._check(self._lib.zoic_tile_set_inputs(self._h, int(inputs)))

    def submit(self, n, ray_index_base=0):
        self._cam._check(self._lib.zoic_tile_submit(self._h, int(n), int(ray_index_base)))

    def wait(self):
        self._cam._check(self._lib.zoic_tile_wait(self._h))

    def done(self):
        return bool(self._lib.zoic_tile_done(self._h))

    def close(self):
        if getattr(self, "_h", None):
            # every view onto the page-locked arrays goes before the arrays do
            self.inputs = self.outputs = self.samples = self.rays = None
            self._lib.zoic_tile_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZoicCamera:
    def __init__(self, device=0):
        self._lib = _capi.load()
        h = C.c_void_p()
        self._h = None
        self._check(self._lib.zoic_camera_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.params = None
        self._tiles = weakref.WeakSet()   # the ZoicTile objects made by tile(): closed with the camera

    # ------------------------------------------------------------------ lifetime
    def _check(self, status):
        if status != 0:
            raise ZoicError(status, (self._lib.zoic_last_error_string() or b"").decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            for t in list(getattr(self, "_tiles", ())):
                t.close()
            self._lib.zoic_camera_destroy(self._h)   # (would settle and detach them itself: the C-ABI's own rule, include/zoic_amd.h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ arguments of the batch calls
    def _device_tensor(self, name, t, shape, ints=False, missing=ValueError):
        """t, if it is what every tensor argument of a batch call must be: a torch tensor (else `missing` is raised: TypeError for
        wavelengths), float32 (ints: int32 or uint32), of exactly `shape` (None: a free dimension), contiguous, on the camera's
        device.  Anything else is a ValueError: the kernels read and write through the bare pointer."""
        import torch
        if not _is_torch(t):
            raise missing("%s must be a torch tensor on cuda:%d, as the items are (numpy arrays go with numpy items)" % (name, self.device))
        s = t.shape
        if (t.dtype not in ((torch.int32, torch.uint32) if ints else (torch.float32,)) or not t.is_contiguous() or not t.is_cuda
                or t.device.index != self.device
                or (s != shape and (len(s) != len(shape) or any(w is not None and w != g for w, g in zip(shape, s))))):
            raise ValueError("%s must be a contiguous (%s) %s tensor on cuda:%d, this camera's device; it is a %s(%s) %s tensor on %s"
                             % (name, ",".join("*" if w is None else str(w) for w in shape), "int32/uint32" if ints else "float32", self.device,
                                "" if t.is_contiguous() else "strided ", ",".join(str(g) for g in s), str(t.dtype).replace("torch.", ""), t.device))
        return t

    def _result(self, name, t, shape, like, ints=False):
        """the tensor a batch call writes into: a new one on like's device, or the caller's, checked"""
        if t is None:
            import torch
            return torch.empty(shape, dtype=torch.int32 if ints else torch.float32, device=like.device)
        return self._device_tensor(name, t, shape, ints)

    def _rng_pointer(self, rng_states, n):
        return None if rng_states is None else self._device_tensor("rng_states", rng_states, (n, 4), ints=True).data_ptr()

    def _traced(self, n, rays, rng_states, lead=None):
        """(the record tensor, the rng_states pointer) of a call that follows a forward call on n samples: rays -- its records, or
        its dict, of shape lead + (8,) (None: (n,)) -- and rng_states as that call was given them"""
        return self._device_tensor("rays", _records(rays), ((n,) if lead is None else lead) + (8,)), self._rng_pointer(rng_states, n)

    def _wavelength_pointer(self, wavelengths, n):
        return None if wavelengths is None else self._device_tensor("wavelengths", wavelengths, (n,), missing=TypeError).data_ptr()

    def _stream(self, stream):
        """the stream argument of a device call: the caller's handle, or torch's current stream on the camera's device"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
        return C.c_void_p(stream)

    def _spectral_or(self, dline, spectral, wavelength, head, tail):
        """dline(h, *head, *tail), or with a wavelength (a float, or the pointer of one per item) spectral(h, *head, wavelength, *tail):
        how every d-line entry point of the C-ABI and its spectral twin take their arguments"""
        if wavelength is None:
            self._check(dline(self._h, *head, *tail))
        else:
            self._check(spectral(self._h, *head, wavelength, *tail))

    def _through_device(self, what, width, items, others, results, probe, half):
        """The numpy half of a batch call: what the torch half `half` returns for the arrays copied to the camera's device, complete
        (the device has been waited for); the caller turns it into numpy.

        items: the (n, width) float32 `what` (width 8: (n,) zoic_ray records too); others: (name, array or None, normaliser) of the
        further arrays; results: name -> the caller's result buffer, which must be None here; probe(*host arrays): the library call
        with no pointers that reports a tables-only camera (ZOIC_ERR_NO_DEVICE); half(*device tensors)."""
        if any(r is not None for r in results.values()):
            raise ValueError("%s are for torch %s" % (", ".join(results), what))
        if any(_is_torch(a) for _, a, _ in others):
            raise TypeError("numpy %s need numpy %s" % (what, ", ".join(name for name, _, _ in others)))
        a = np.asarray(items)
        if width == 8 and a.dtype == np.dtype(_capi.RAY_DTYPE):
            a = np.ascontiguousarray(a).reshape(-1).view(np.float32).reshape(-1, 8)
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError("%s must be (n, %d)%s" % (what, width, " float32 or (n,) zoic_ray records" if width == 8 else ""))
        host = [a] + [None if v is None else norm(v, a.shape[0]) for _, v, norm in others]
        if self.device < 0:
            self._check(probe(*host))
        import torch
        dev = torch.device("cuda", self.device)
        res = half(*[None if v is None else torch.from_numpy(v).to(dev) for v in host])
        torch.cuda.synchronize(dev)
        return res

    # ------------------------------------------------------------------ node_update
    def set_bokeh_image(self, pixels):
        """pixels: (H, W, C>=3) float32 -- what AiTextureLoad would return for bokehPath (zoic.cpp:176-186)."""
        px = np.ascontiguousarray(pixels, dtype=np.float32)
        if px.ndim != 3:
            raise ValueError("bokeh image must be (H, W, C)")
        h, w, c = px.shape
        self._check(self._lib.zoic_camera_set_bokeh_image(self._h, w, h, c, px.ctypes.data))

    def set_lens_text(self, text):
        if text is None:
            self._check(self._lib.zoic_camera_set_lens_text(self._h, None, 0))
            return
        b = text.encode() if isinstance(text, str) else bytes(text)
        self._check(self._lib.zoic_camera_set_lens_text(self._h, b, len(b)))

    def set_precision(self, mode):
        self._check(self._lib.zoic_camera_set_precision(self._h, int(mode)))

    def set_wait_mode(self, mode):
        """0 spin (default), 1 yield, 2 sleep: how a calling thread waits for the resident kernel (zoic_camera_set_wait_mode)."""
        self._check(self._lib.zoic_camera_set_wait_mode(self._h, int(mode)))

    def set_seed(self, seed):
        self._check(self._lib.zoic_camera_set_seed(self._h, int(seed) & 0xFFFFFFFF))

    def set_frame_aspect(self, max_abs_sy):
        """The largest |sy| the renderer sends (1/aspect): the extent node_update's self-check of the FAST modes probes."""
        self._check(self._lib.zoic_camera_set_frame_aspect(self._h, float(max_abs_sy)))

    def update(self, **kw):
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise KeyError("unknown zoic parameter(s): %s" % sorted(unknown))
        p = dict(DEFAULTS)
        p.update(kw)
        P = _capi.Params()
        self._keep = []
        for k, v in p.items():
            if k in _STR:
                b = str(v).encode()
                self._keep.append(b)
                setattr(P, k, b)
            elif k in _INT:
                setattr(P, k, int(v))
            else:
                setattr(P, k, float(v))
        self.params = p
        self._check(self._lib.zoic_camera_update(self._h, C.byref(P)))
        return self

    # ------------------------------------------------------------------ camera_create_ray
    def create_rays(self, samples, rng_states=None, ray_index_base=0, out=None, stream=None, wavelengths=None):
        """samples: (n,4) float32 rows (sx, sy, lensx, lensy).

        numpy in  -> host API (H2D, kernels, D2H); returns a dict of numpy arrays built from the (n,) zoic_ray records:
                     rays (structured), planes (7,n) = ox oy oz dx dy dz weight, origin (3,n), dir (3,n), weight, flags, tries.
        torch device tensor in -> device API, asynchronous on `stream` (default: torch's current stream); returns a dict
                     with rays = (n,8) float32 tensor (column 7 holds the flag word's bits) and strided views into it.
        wavelengths: None (the d-line path above, untouched) or n float32 wavelengths in nm, one per ray
                     (zoic_create_rays_spectral_device).  With torch samples a (n,) float32 device tensor, asynchronous as above;
                     with numpy samples a numpy array: samples, wavelengths and rng_states are copied to the camera's device through
                     torch, the call waits for the records and returns the numpy dict (out must be None there).
        """
        if _is_torch(samples):
            return self._create_rays_torch(samples, wavelengths, False, rng_states, ray_index_base, out, stream)
        if wavelengths is not None:
            res = self._through_device(
                "samples", 4, samples, [("wavelengths", wavelengths, _f32_flat), ("rng_states", rng_states, _rng_words)], dict(out=out),
                lambda s, w, r: self._lib.zoic_create_rays_spectral_device(self._h, len(s), None, None, None, int(ray_index_base), None, None),
                lambda s, w, r: self._create_rays_torch(s, w, False, r, ray_index_base, None, None))
            return rays_to_dict(_host_records(res["rays"]))
        s = np.ascontiguousarray(samples, dtype=np.float32)
        if s.ndim != 2 or s.shape[1] != 4:
            raise ValueError("samples must be (n, 4)")
        n = s.shape[0]
        if out is not None:   # caller-owned (e.g. pinned) record array
            rays = out
            if rays.dtype != np.dtype(_capi.RAY_DTYPE) or rays.shape != (n,) or not rays.flags.c_contiguous:
                raise ValueError("out must be an (n,) C-contiguous array of zoic_ray records")
        else:
            rays = np.empty(n, dtype=_capi.RAY_DTYPE)
        rs_ptr = None
        if rng_states is not None:
            rs = np.ascontiguousarray(rng_states, dtype=np.uint32)
            if rs.shape != (n, 4):
                raise ValueError("rng_states must be (n, 4) uint32")
            rs_ptr = rs.ctypes.data
        self._check(self._lib.zoic_create_rays_host(self._h, n, s.ctypes.data, rs_ptr, int(ray_index_base), rays.ctypes.data))
        return rays_to_dict(rays)

    def _create_rays_torch(self, samples, wavelengths, hero, rng_states, ray_index_base, out, stream):
        """the torch half of create_rays (wavelengths None or (n,)) and of create_rays_hero (hero: wavelengths (n,k))"""
        n = self._device_tensor("samples", samples, (None, 4)).shape[0]
        lead = (n,)
        if hero or wavelengths is not None:
            lead = tuple(self._device_tensor("wavelengths", wavelengths, (n, None) if hero else (n,), missing=TypeError).shape)
        out = dict(rays=None) if out is None else out
        rays = out["rays"] = self._result("out['rays']", out["rays"], lead + (8,), samples)
        tail = (self._rng_pointer(rng_states, n), int(ray_index_base), rays.data_ptr(), self._stream(stream))
        if wavelengths is None:
            self._check(self._lib.zoic_create_rays_device(self._h, n, samples.data_ptr(), *tail))
        elif hero:
            self._check(self._lib.zoic_create_rays_hero_device(self._h, n, lead[1], samples.data_ptr(), wavelengths.data_ptr(), *tail))
        else:
            self._check(self._lib.zoic_create_rays_spectral_device(self._h, n, samples.data_ptr(), wavelengths.data_ptr(), *tail))
        out.update(_ray_views(rays))
        return out

    def create_rays_hero(self, samples, wavelengths, rng_states=None, ray_index_base=0, out=None, stream=None):
        """Hero-wavelength rays (zoic_create_rays_hero_device): k wavelengths through one lens point per sample.

        samples: (n, 4) float32; wavelengths: (n, k) float32 in nm, the hero in column 0, 1 <= k <= HERO_MAX_WAVELENGTHS.  Column 0 of
        the result is create_rays(samples, wavelengths=wavelengths[:, 0]); column j >= 1 is the hero's accepted start traced at
        wavelengths[:, j], or a lost record (zeros, weight 0, the hero's flags | RAY_COMPANION_LOST).
        torch device tensors in -> asynchronous on `stream` (default: torch's current stream); returns a dict with rays = (n, k, 8)
                     float32 tensor (word 7 holds the flag word's bits) and strided views: origin, dir (3, n, k), planes (7, n, k),
                     weight (n, k), flags (n, k) int32.
        numpy in  -> samples, wavelengths and rng_states are copied to the camera's device through torch, the call waits and returns
                     numpy arrays of those shapes with a structured (n, k) rays (out must be None there).
        """
        if _is_torch(samples):
            return self._create_rays_torch(samples, wavelengths, True, rng_states, ray_index_base, out, stream)
        res = self._through_device(
            "samples", 4, samples, [("wavelengths", wavelengths, _hero_wavelengths), ("rng_states", rng_states, _rng_words)], dict(out=out),
            lambda s, w, r: self._lib.zoic_create_rays_hero_device(self._h, len(s), w.shape[1], None, None, None, int(ray_index_base), None, None),
            lambda s, w, r: self._create_rays_torch(s, w, True, r, ray_index_base, None, None))
        return hero_rays_to_dict(_host_records(res["rays"]))

    def dispersion(self):
        """The lens's dispersion table (zoic_camera_get_dispersion), trace order (rear first): dict of float32 arrays ior_d, abbe and
        cauchy_b (nm^2).  Works on a tables-only camera (device=-1)."""
        return self._table(self._lib.zoic_camera_get_dispersion, np.float32, ("ior_d", "abbe", "cauchy_b"))

    def _table(self, getter, dtype, names):
        """the arrays of a table getter of the C-ABI, by name: ask for the size (no pointers), then have one array per name filled"""
        n = getter(self._h, 0, *[None] * len(names))
        if n < 0:
            self._check(1)   # ZOIC_ERR_INVALID_ARGUMENT with the library's detail
        a = {k: np.zeros(n, dtype=dtype) for k in names}
        getter(self._h, n, *[v.ctypes.data for v in a.values()])
        return a

    def set_abbe_numbers(self, V):
        """V-numbers in FILE order (front to rear, as the prescription lists them) for the dispersion table; None clears them."""
        if V is None:
            self._check(self._lib.zoic_camera_set_abbe_numbers(self._h, 0, None))
            return
        v = np.ascontiguousarray(V, dtype=np.float32).reshape(-1)
        self._check(self._lib.zoic_camera_set_abbe_numbers(self._h, v.shape[0], v.ctypes.data))

    def create_rays_device_ptr(self, n, d_samples, d_rays, d_rng=None, ray_index_base=0, stream=0):
        """Raw-pointer form of zoic_create_rays_device (d_rays: n x 32-byte zoic_ray records)."""
        self._check(self._lib.zoic_create_rays_device(self._h, n, d_samples, d_rng, int(ray_index_base), d_rays,
                                                      C.c_void_p(stream)))

    def create_rays_resident(self, samples, ray_index_base=0, out=None, tid=0):
        """(n, 4) float32 samples on the camera's device -> (n, 8) float32 zoic_ray records on the device through the RESIDENT kernel
        (zoic_create_rays_device_resident): no launch, not stream-ordered -- the current stream is synchronised first (the samples must
        be complete), the records are complete on return.  The bits of create_rays(samples, ray_index_base=...)."""
        import torch
        n = self._device_tensor("samples", samples, (None, 4)).shape[0]
        out = self._result("out", out, (n, 8), samples)
        torch.cuda.current_stream(samples.device).synchronize()
        self._check(self._lib.zoic_create_rays_device_resident(self._h, n, samples.data_ptr(), out.data_ptr(), int(ray_index_base), int(tid) & 0xFFFF))
        return out

    def create_ray(self, sx, sy, lensx, lensy, tid=0):
        """The per-sample camera_create_ray(node, input, output, tid) signature (one AtCameraInput in, one AtCameraOutput out)."""
        i = _capi.CameraInput(sx, sy, 0.0, 0.0, lensx, lensy, 0.0)
        o = _capi.CameraOutput()
        o.weight[0] = o.weight[1] = o.weight[2] = 1.0
        self._check(self._lib.zoic_camera_create_ray(self._h, C.byref(i), C.byref(o), int(tid)))
        return o

    def reverse_ray(self, Po=(0.0, 0.0, 0.0), fov=0.0):
        """camera_reverse_ray (zoic.cpp:1992-1995): False, nothing written -- unless set_reverse_projection(True): then whether Po
        projects (zoic_project_point's flag bit 0)."""
        po = _capi.Vec3(*[float(v) for v in Po])
        ps = (C.c_float * 2)(0.0, 0.0)
        t = C.c_float(0.0)
        return bool(self._lib.zoic_camera_reverse_ray(self._h, C.byref(po), float(fov), ps, C.byref(t)))

    def set_reverse_projection(self, enable):
        """Opt in (True) or out (False, the default) of answering reverse_ray / camera_reverse_ray with the projection."""
        self._check(self._lib.zoic_camera_set_reverse_projection(self._h, 1 if enable else 0))

    def _backward_batch(self, what, width, dline, spectral, items, wavelengths, out, flags, stream, jacobian=None, with_jacobian=False):
        """The batch wrapper of project_points, trace_back and trace_back_jacobian.  `what` ("points" / "rays") names the (n, width)
        float32 items; dline / spectral are the library's entry points without and with wavelengths.  Returns (out, flags) and, with
        with_jacobian, the (n,2,6) jacobian: tensors for torch items, numpy arrays (after a round trip and a wait) for numpy items."""
        more = 1 if with_jacobian else 0
        if not _is_torch(items):
            res = self._through_device(
                what, width, items, [("wavelengths", wavelengths, _f32_flat)], dict(out=out, flags=flags, **(dict(jacobian=jacobian) if more else {})),
                lambda a, w: dline(self._h, len(a), *[None] * (4 + more)) if w is None else spectral(self._h, len(a), *[None] * (5 + more)),
                lambda t, w: self._backward_batch(what, width, dline, spectral, t, w, None, None, None, None, with_jacobian))
            return tuple(t.cpu().numpy() for t in res)
        n = self._device_tensor(what, items, (None, width)).shape[0]
        res = [self._result("out", out, (n, 2), items), self._result("flags", flags, (n,), items, ints=True)]
        if with_jacobian:
            res.append(self._result("jacobian", jacobian, (n, 2, 6), items))
        w = self._wavelength_pointer(wavelengths, n)
        self._spectral_or(dline, spectral, w, (n, items.data_ptr()), [t.data_ptr() for t in res] + [self._stream(stream)])
        return tuple(res)

    def _screen_sample(self, dline, spectral, vectors, wavelength, *extra):
        """the host single-item wrappers' call: the (sx, sy, flags) both entry points write for `vectors` (a point, or an origin and
        a dir); extra: further output arguments of both"""
        ps = (C.c_float * 2)(0.0, 0.0)
        f = C.c_uint32(0)
        self._spectral_or(dline, spectral, None if wavelength is None else float(wavelength),
                          [C.byref(_capi.Vec3(*[float(x) for x in v])) for v in vectors], (ps, C.byref(f)) + extra)
        return float(ps[0]), float(ps[1]), int(f.value)

    def project_point(self, Po, wavelength=None):
        """Reverse projection of one point on the host (zoic_project_point): (sx, sy, flags).  Po in the frame of the records the
        forward calls write.  flags bit 0: projected; bit 1: the chief ray is clipped; bit 2: beyond the exit-pupil LUT; bits 8-11:
        the reason a point is not projected (csrc/reverse.hpp).  Works on a tables-only camera (device=-1).
        wavelength (nm): the projection through the glass at that wavelength (zoic_project_point_spectral, csrc/backward_spectral.hpp);
        outside [360, 830] or NaN: not projected, reason _capi.PROJECT_WAVELENGTH."""
        return self._screen_sample(self._lib.zoic_project_point, self._lib.zoic_project_point_spectral, (Po,), wavelength)

    def project_points(self, points, out=None, flags=None, stream=None, wavelengths=None):
        """Reverse projection of (n,3) float32 points (zoic_project_points_device): returns (screen (n,2) float32, flags (n,) int32).

        numpy in  -> the points are copied to the camera's device through torch, the call waits and returns numpy arrays (out and
                     flags must be None there).
        torch device tensor in -> asynchronous on `stream` (default: torch's current stream); out / flags: optional (n,2) float32 and
                     (n,) int32 tensors on the points' device to write into.
        wavelengths: (n,) float32 (nm), numpy with numpy points, a device tensor with device points: every point projected at its own
                     wavelength (zoic_project_points_spectral_device); None: the d-line call."""
        return self._backward_batch("points", 3, self._lib.zoic_project_points_device, self._lib.zoic_project_points_spectral_device, points,
                                    wavelengths, out, flags, stream)

    def trace_back_ray(self, origin, dir, wavelength=None):
        """Trace-back of one camera ray on the host (zoic_trace_back_ray): (sx, sy, flags).  origin / dir in the frame of the records
        the forward calls write, dir pointing into the scene (any length).  flags bit 0: the ray reaches the sensor unclipped; bit 2:
        beyond the exit-pupil LUT; bits 8-11: why not; bits 16-21: the interface where it ended (csrc/traceback.hpp).  Works on a
        tables-only camera (device=-1).
        wavelength (nm): the trace through the glass at that wavelength (zoic_trace_back_ray_spectral, csrc/backward_spectral.hpp);
        outside [360, 830] or NaN: not traced back, reason _capi.TRACE_BACK_WAVELENGTH."""
        return self._screen_sample(self._lib.zoic_trace_back_ray, self._lib.zoic_trace_back_ray_spectral, (origin, dir), wavelength)

    def trace_back(self, rays, out=None, flags=None, stream=None, wavelengths=None):
        """Trace-back of n camera rays (zoic_trace_back_rays_device): returns (screen (n,2) float32, flags (n,) int32).

        rays: an (n,8) float32 device tensor of zoic_ray records, or the dict a create_rays call on device tensors returned (its
                     "rays" buffer is read in place) -> asynchronous on `stream` (default: torch's current stream); out / flags:
                     optional (n,2) float32 and (n,) int32 tensors on the rays' device to write into.
        numpy in  -> (n,) zoic_ray records (or the dict of a numpy create_rays call) or an (n,8) float32 array: copied to the camera's
                     device through torch, the call waits and returns numpy arrays (out and flags must be None there).
        wavelengths: (n,) float32 (nm), numpy with numpy rays, a device tensor with device rays -- for the records of
                     create_rays(samples, wavelengths=w), the same w: every ray traced back at its own wavelength
                     (zoic_trace_back_rays_spectral_device); None: the d-line call."""
        return self._backward_batch("rays", 8, self._lib.zoic_trace_back_rays_device, self._lib.zoic_trace_back_rays_spectral_device,
                                    _records(rays), wavelengths, out, flags, stream)

    def trace_back_ray_jacobian(self, origin, dir, wavelength=None):
        """Trace-back of one camera ray on the host with its Jacobian (zoic_trace_back_ray_jacobian): (sx, sy, flags, J (2,6) float32).
        sx, sy and flags are trace_back_ray's bit for bit; J = d(sx, sy) / d(origin.xyz, dir.xyz), dir differentiated as given
        (csrc/traceback_jacobian.hpp); all zero for a ray that is not traced back.  Works on a tables-only camera (device=-1).
        wavelength (nm): the trace at that wavelength, held fixed (zoic_trace_back_ray_jacobian_spectral)."""
        jac = np.zeros((2, 6), np.float32)
        return self._screen_sample(self._lib.zoic_trace_back_ray_jacobian, self._lib.zoic_trace_back_ray_jacobian_spectral, (origin, dir),
                                   wavelength, jac.ctypes.data_as(C.POINTER(C.c_float))) + (jac,)

    def trace_back_jacobian(self, rays, wavelengths=None, out=None, flags=None, jacobian=None, stream=None):
        """Trace-back of n camera rays with the Jacobian of each (zoic_trace_back_jacobian_device): returns (screen (n,2) float32,
        flags (n,) int32, jac (n,2,6) float32).  screen and flags are trace_back's bit for bit; jac[i] = d(sx, sy) / d(origin.xyz,
        dir.xyz) of ray i (csrc/traceback_jacobian.hpp), all zero where bit 0 of its flags is clear.  solid_angle_measure(jac, dirs)
        turns it into the dPs/d(omega) a splatter divides by.

        rays, wavelengths, stream: as trace_back takes them (device tensors, the dict of a create_rays call, or numpy).
        out / flags / jacobian: optional (n,2) float32, (n,) int32 and (n,2,6) float32 tensors on the rays' device to write into
        (torch rays only)."""
        return self._backward_batch("rays", 8, self._lib.zoic_trace_back_jacobian_device, self._lib.zoic_trace_back_jacobian_spectral_device,
                                    _records(rays), wavelengths, out, flags, stream, jacobian, True)

    @staticmethod
    def _pupil_window(window):
        """the window argument of the pupil-bounds calls: None, or four floats (sx0, sy0, sx1, sy1) of host memory"""
        if window is None:
            return None
        w = [float(v) for v in window]
        if len(w) != 4:
            raise ValueError("window must be (sx0, sy0, sx1, sy1)")
        return (C.c_float * 4)(*w)

    def pupil_square(self):
        """(z, R) of the square [-R, R]^2 the pupil-bounds aims lie in, in the frame of the records: RAYTRACED the front vertex plane
        and the front element's housing radius, THINLENS the lens plane z = 0 and apertureRadius (csrc/pupil_bounds.hpp, in the
        table's own f32 operations).  4 R^2 count / lattice of a pupil-bounds record is the pupil's area as seen from its point;
        z is the aim_z of pupil_rays."""
        info, f32 = self.info(), np.float32
        if int(self.params["lensModel"]) != RAYTRACED:
            a = f32(info["apertureRadius"])
            return 0.0, float(np.sqrt(f32(a * a)))
        n = int(info["lensCount"])
        th = info["elements"][:n, 1].astype(f32)
        front = th[0]
        for t in th[1:]:
            front = f32(front + t)
        lim = (float(info["elements"][n - 1, 3]) * 0.5) ** 2
        h2 = f32(lim)
        if float(h2) > lim:
            h2 = np.nextafter(h2, f32(-np.inf))
        ua = f32(info["userApertureRadius"])
        if info["apertureElement"] == n - 1 and f32(ua * ua) < h2:
            h2 = f32(ua * ua)
        return -float(front), float(np.sqrt(h2))

    def pupil_bounds_point(self, Po, lattice=16, window=None, wavelength=None):
        """Pupil bounds of one scene point on the host (zoic_pupil_bounds_point): a dict with aim (4,) float32 = (min ax, min ay, max ax,
        max ay), the box of the lattice aims whose rays from Po are traced back, grown by a pitch; screen (4,) float32 = (min sx, min sy,
        max sx, max sy), the box of the blur spot; count, lattice (= lattice^2) and flags (csrc/pupil_bounds.hpp).  Po in the frame of
        the records; lattice 8, 16 or 32; window: None or (sx0, sy0, sx1, sy1), the film window an aim's sample must land in.  Works
        on a tables-only camera (device=-1).
        wavelength (nm): the trace at that wavelength (zoic_pupil_bounds_point_spectral)."""
        po = _capi.Vec3(*[float(v) for v in Po])
        b = _capi.PupilBounds()
        w = self._pupil_window(window)
        self._spectral_or(self._lib.zoic_pupil_bounds_point, self._lib.zoic_pupil_bounds_point_spectral,
                          None if wavelength is None else float(wavelength), (C.byref(po),), (int(lattice), w, C.byref(b)))
        return dict(aim=np.array(b.aim[:], np.float32), screen=np.array(b.screen[:], np.float32), count=int(b.count), lattice=int(b.lattice),
                    flags=int(b.flags))

    def pupil_bounds(self, points, lattice=16, window=None, wavelengths=None, out=None, stream=None):
        """Pupil bounds of (n,3) float32 scene points (zoic_pupil_bounds_device): for each point the box of the lens it sees and the box
        of its blur spot, from a lattice x lattice grid of aims on the front element traced back from the point (csrc/pupil_bounds.hpp).

        numpy in  -> the points are copied to the camera's device through torch, the call waits and returns an (n,) structured array
                     (_capi.PUPIL_BOUNDS_DTYPE: aim (4,), screen (4,), count, lattice, flags, reserved); out must be None there.
        torch device tensor in -> asynchronous on `stream` (default: torch's current stream); returns the records as an (n,12) float32
                     device tensor (columns 0-3 aim, 4-7 screen, 8-11 the bits of count, lattice, flags, reserved: view them as int32);
                     out: an optional tensor of that kind to write into.  pupil_bounds_records(t) turns it into the structured array.
        lattice: 8, 16 or 32.  window: None or (sx0, sy0, sx1, sy1).
        wavelengths: (n,) float32 (nm), numpy with numpy points, a device tensor with device points (zoic_pupil_bounds_spectral_device)."""
        w = self._pupil_window(window)
        if not _is_torch(points):
            res = self._through_device("points", 3, points, [("wavelengths", wavelengths, _f32_flat)], dict(out=out),
                                       lambda a, lam: self._lib.zoic_pupil_bounds_device(self._h, len(a), None, int(lattice), w, None, None),
                                       lambda t, lam: self.pupil_bounds(t, lattice, window, lam))
            return pupil_bounds_records(res)
        n = self._device_tensor("points", points, (None, 3)).shape[0]
        out = self._result("out", out, (n, 12), points)
        lam = self._wavelength_pointer(wavelengths, n)
        self._spectral_or(self._lib.zoic_pupil_bounds_device, self._lib.zoic_pupil_bounds_spectral_device, lam, (n, points.data_ptr()),
                          (int(lattice), w, out.data_ptr(), self._stream(stream)))
        return out

    def splat_point(self, Po, bounds, u, wavelength=None):
        """Lens splats of one scene point on the host (zoic_splat_point): the (m,) structured array (_capi.SPLAT_DTYPE) of the m rays
        from Po towards the aims u (m,2) picks in the box of `bounds` -- the dict pupil_bounds_point returned, or one record of
        pupil_bounds (structured, or its 12 float32).  Each record: the screen sample (sx, sy), the aim (ax, ay), area =
        det d(sx, sy)/d(ax, ay), angle = dPs/d(omega) and the trace-back's flags, or _capi.SPLAT_NO_BOX for an empty box
        (csrc/splat.hpp).  Draws nothing: u is the caller's.  Works on a tables-only camera (device=-1).
        wavelength (nm): the trace at that wavelength (zoic_splat_point_spectral)."""
        return self._splat_item(self._lib.zoic_splat_point, self._lib.zoic_splat_point_spectral, Po, bounds, u, wavelength, _capi.SPLAT_DTYPE)

    def _splat_item(self, dline, spectral, Po, bounds, u, wavelength, dtype):
        """the host single-point wrappers' call of the splat family: the (m,) array of `dtype` both entry points write for Po, its
        bounds (the dict of pupil_bounds_point, or one record) and the aims u (m,2)"""
        po = _capi.Vec3(*[float(v) for v in Po])
        if isinstance(bounds, dict):
            rec = np.zeros(1, _capi.PUPIL_BOUNDS_DTYPE)
            rec[0] = (bounds["aim"], bounds["screen"], bounds["count"], bounds["lattice"], bounds["flags"], 0)
        else:
            rec = pupil_bounds_records(bounds)
            if len(rec) != 1:
                raise ValueError("bounds must be one pupil-bounds record")
        b = _capi.PupilBounds.from_buffer_copy(rec.tobytes())
        uu = np.ascontiguousarray(u, dtype=np.float32)
        if uu.ndim != 2 or uu.shape[1] != 2:
            raise ValueError("u must be (m, 2)")
        m = uu.shape[0]
        out = np.zeros(m, dtype)
        up, op = uu.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        self._spectral_or(dline, spectral, None if wavelength is None else float(wavelength), (C.byref(po), C.byref(b)), (m, up, op))
        return out

    def splat_points(self, points, bounds, u, wavelengths=None, out=None, stream=None):
        """Lens splats of (n,3) float32 scene points (zoic_splat_points_device): m rays per point towards aims in the point's pupil
        box, each traced back with its Jacobian; per ray one 32-byte record (sx, sy, ax, ay, area, angle, flags, reserved) with the
        screen sample, the aim, area = det d(sx, sy)/d(ax, ay) (screen area per cm^2 of the aims' plane) and angle = dPs/d(omega)
        (csrc/splat.hpp).  The device pipeline of a splatter is pupil_bounds -> splat_points -> the caller's own weights and
        accumulation; nothing is drawn here: u (n,m,2) float32 are the caller's numbers in [0,1)^2.

        torch device tensors in -> asynchronous on `stream` (default: torch's current stream); bounds: the (n,12) float32 tensor
                     pupil_bounds returned, read in place; returns the records as an (n,m,8) float32 device tensor (column 6 holds
                     the bits of flags: view it as int32); out: an optional tensor of that kind to write into.  splat_records(t)
                     turns it into the structured array.
        numpy in  -> points, bounds (the structured records or (n,12) float32) and u are copied to the camera's device through
                     torch, the call waits and returns an (n,m) structured array (_capi.SPLAT_DTYPE); out must be None there.
        wavelengths: (n,) float32 (nm), numpy with numpy points, a device tensor with device points (zoic_splat_points_spectral_device)."""
        if not _is_torch(points):
            res = self._through_device(
                "points", 3, points, [("bounds", bounds, _bounds_floats), ("u", u, _f32), ("wavelengths", wavelengths, _f32_flat)], dict(out=out),
                lambda a, b, uu, lam: self._lib.zoic_splat_points_device(self._h, len(a), None, None, 1, None, None, None),
                lambda t, b, uu, lam: self.splat_points(t, b, uu, lam))
            return splat_records(res)
        n = self._device_tensor("points", points, (None, 3)).shape[0]
        self._device_tensor("bounds", bounds, (n, 12))
        m = self._device_tensor("u", u, (n, None, 2)).shape[1]
        if m < 1:
            raise ValueError("u must hold at least one aim per point: (n,m,2), m >= 1")
        out = self._result("out", out, (n, m, 8), points)
        lam = self._wavelength_pointer(wavelengths, n)
        self._spectral_or(self._lib.zoic_splat_points_device, self._lib.zoic_splat_points_spectral_device, lam,
                          (n, points.data_ptr(), bounds.data_ptr()), (m, u.data_ptr(), out.data_ptr(), self._stream(stream)))
        return out

    def trace_back_ray_transmittance(self, origin, dir, wavelength=None):
        """Trace-back of one camera ray on the host with its Fresnel transmittance (zoic_trace_back_ray_transmittance): (sx, sy, flags,
        T).  sx, sy and flags are trace_back_ray's bit for bit; T is the share of unpolarised light the interfaces let through along
        that path, front to rear, bare or with the films of set_coatings: in (0, 1] where flags bit 0 is set, +0.0 otherwise; 1.0
        for a traced THINLENS ray (csrc/traceback_throughput.hpp).  Works on a tables-only camera (device=-1).
        wavelength (nm): the trace and the films at that wavelength (zoic_trace_back_ray_transmittance_spectral); None: the d-line."""
        t = C.c_float(0.0)
        return self._screen_sample(self._lib.zoic_trace_back_ray_transmittance, self._lib.zoic_trace_back_ray_transmittance_spectral,
                                   (origin, dir), wavelength, C.byref(t)) + (float(t.value),)

    def trace_back_transmittance(self, rays, wavelengths=None, out=None, screen=None, flags=None, stream=None):
        """Trace-back of n camera rays with the Fresnel transmittance of each backward path (zoic_trace_back_transmittance_device):
        returns (T (n,) float32, screen (n,2) float32, flags (n,) int32).  screen and flags are trace_back's bit for bit; T[i] is in
        (0, 1] where bit 0 of flags[i] is set and +0.0 elsewhere (csrc/traceback_throughput.hpp).  For the records of a forward call
        T equals what transmittance() gives for them, to rounding.  The films (set_coatings) and the dispersion (set_abbe_numbers)
        are read at the call.  Multilayer stacks (set_coating_stacks) are honoured where an interface has one.

        rays, wavelengths, stream: as trace_back takes them -- an (n,8) float32 device tensor of zoic_ray records or the dict a
                     create_rays call on device tensors returned (its "rays" buffer is read in place), asynchronous on `stream`
                     (default: torch's current stream); or numpy ((n,) zoic_ray records, the dict of a numpy create_rays call, or an
                     (n,8) float32 array): copied to the camera's device through torch, the call waits and returns numpy arrays.
                     wavelengths: (n,) float32 (nm), numpy with numpy rays, a device tensor with device rays
                     (zoic_trace_back_transmittance_spectral_device); None: the d-line call.
        out / screen / flags: optional (n,) float32, (n,2) float32 and (n,) int32 tensors on the rays' device to write into (torch
                     rays only; they must be None with numpy rays)."""
        lib = self._lib
        rays = _records(rays)
        if not _is_torch(rays):
            res = self._through_device(
                "rays", 8, rays, [("wavelengths", wavelengths, _f32_flat)], dict(out=out, screen=screen, flags=flags),
                lambda a, w: lib.zoic_trace_back_transmittance_device(self._h, len(a), None, None, None, None, None),
                lambda t, w: self.trace_back_transmittance(t, w))
            return tuple(t.cpu().numpy() for t in res)
        n = self._device_tensor("rays", rays, (None, 8)).shape[0]
        res = [self._result("out", out, (n,), rays), self._result("screen", screen, (n, 2), rays),
               self._result("flags", flags, (n,), rays, ints=True)]
        w = self._wavelength_pointer(wavelengths, n)
        self._spectral_or(lib.zoic_trace_back_transmittance_device, lib.zoic_trace_back_transmittance_spectral_device, w,
                          (n, rays.data_ptr()), [t.data_ptr() for t in res] + [self._stream(stream)])
        return tuple(res)

    def splat_point_transmittance(self, Po, bounds, u, wavelength=None):
        """The Fresnel transmittance of the m rays splat_point traces for one scene point, on the host
        (zoic_splat_point_transmittance): (m,) float32, T[j] of the ray from Po towards aim u[j] of the box of `bounds` -- Po, bounds
        and u as splat_point takes them.  In (0, 1] where that splat record has flags bit 0 set, +0.0 elsewhere, _capi.SPLAT_NO_BOX
        records included (csrc/traceback_throughput.hpp).  Works on a tables-only camera (device=-1).
        wavelength (nm): the trace and the films at that wavelength (zoic_splat_point_transmittance_spectral)."""
        return self._splat_item(self._lib.zoic_splat_point_transmittance, self._lib.zoic_splat_point_transmittance_spectral, Po, bounds, u,
                                wavelength, np.float32)

    def splat_transmittance(self, points, bounds, u, wavelengths=None, out=None, stream=None):
        """The Fresnel transmittance of the rays splat_points traces (zoic_splat_transmittance_device): (n,m) float32, entry (p, j) for
        the ray of splat record (p, j) of splat_points(points, bounds, u, wavelengths): in (0, 1] where that record has flags bit 0
        set, +0.0 elsewhere (csrc/traceback_throughput.hpp).  A splatter multiplies each splat's weight by it.
        Multilayer stacks (set_coating_stacks) are honoured where an interface has one.

        points, bounds, u, wavelengths, stream: as splat_points takes them -- torch device tensors ((n,3), the (n,12) tensor
                     pupil_bounds returned, read in place, (n,m,2), (n,)), asynchronous on `stream` (default: torch's current stream);
                     or numpy (bounds: the structured records or (n,12) float32): copied to the camera's device through torch, the
                     call waits and returns a numpy array.
        out: an optional (n,m) float32 tensor on the points' device to write into (torch points only; None with numpy points)."""
        lib = self._lib
        if not _is_torch(points):
            res = self._through_device(
                "points", 3, points, [("bounds", bounds, _bounds_floats), ("u", u, _f32), ("wavelengths", wavelengths, _f32_flat)], dict(out=out),
                lambda a, b, uu, lam: lib.zoic_splat_transmittance_device(self._h, len(a), None, None, 1, None, None, None),
                lambda t, b, uu, lam: self.splat_transmittance(t, b, uu, lam))
            return res.cpu().numpy()
        n = self._device_tensor("points", points, (None, 3)).shape[0]
        self._device_tensor("bounds", bounds, (n, 12))
        m = self._device_tensor("u", u, (n, None, 2)).shape[1]
        if m < 1:
            raise ValueError("u must hold at least one aim per point: (n,m,2), m >= 1")
        out = self._result("out", out, (n, m), points)
        lam = self._wavelength_pointer(wavelengths, n)
        self._spectral_or(lib.zoic_splat_transmittance_device, lib.zoic_splat_transmittance_spectral_device, lam,
                          (n, points.data_ptr(), bounds.data_ptr()), (m, u.data_ptr(), out.data_ptr(), self._stream(stream)))
        return out

    def create_rays_arnold(self, inputs, ray_index_base=0, differentials=False):
        """inputs: (n,7) float32 AtCameraInput rows -> (n,21) float32 AtCameraOutput rows (weight initialised to 1).

        differentials=True: zoic_create_rays_arnold_differentials -- the same origin / dir / weight, and traced dOdx, dOdy, dDdx,
        dDdy (columns 6-17) scaled by each row's dsx / dsy (columns 2, 3) instead of the reference's placeholders."""
        a = np.ascontiguousarray(inputs, dtype=np.float32)
        n = a.shape[0]
        outs = np.zeros((n, 21), dtype=np.float32)
        outs[:, 18:21] = 1.0
        fn = self._lib.zoic_create_rays_arnold_differentials if differentials else self._lib.zoic_create_rays_arnold
        self._check(fn(self._h, n, a.ctypes.data_as(C.POINTER(_capi.CameraInput)), outs.ctypes.data_as(C.POINTER(_capi.CameraOutput)),
                       int(ray_index_base)))
        return outs

    def ray_differentials(self, samples, rays, dsx=1.0, dsy=1.0, rng_states=None, ray_index_base=0, out=None, stream=None,
                          wavelengths=None, chromatic=False):
        """Traced ray differentials (zoic_ray_differentials_device) of rays create_rays made from device tensors.

        samples, rng_states, ray_index_base: what that create_rays call was given; rays: the (n,8) float32 record tensor it returned
        (or its result dict).  The camera must not have been updated in between.  Returns an (n,12) float32 device tensor, columns
        dOdx, dOdy, dDdx, dDdy (x y z each), scaled by dsx / dsy (1: the raw Jacobian columns); asynchronous on `stream` (default:
        torch's current stream).  Rays of weight 0 get zeros.
        wavelengths: None (the d-line call above, untouched) or the (n,) float32 device tensor create_rays(..., wavelengths=) was
        given: the differentials of those spectral records (zoic_ray_differentials_spectral_device); rows whose wavelength is
        outside [360, 830] or NaN get zeros.  chromatic=True (needs wavelengths) returns (diffs, chroma): chroma is an (n,6) float32
        tensor, dO/dlambda and dD/dlambda per nanometre with the sensor point and the lens point held fixed (never scaled by dsx /
        dsy; csrc/differentials_spectral.hpp)."""
        if chromatic and wavelengths is None:
            raise ValueError("chromatic=True needs wavelengths")
        n = self._device_tensor("samples", samples, (None, 4)).shape[0]
        rays, rs_ptr = self._traced(n, rays, rng_states)
        out = self._result("out", out, (n, 12), samples)
        if wavelengths is None:
            self._check(self._lib.zoic_ray_differentials_device(self._h, n, samples.data_ptr(), rs_ptr, int(ray_index_base), rays.data_ptr(),
                                                                float(dsx), float(dsy), out.data_ptr(), self._stream(stream)))
            return out
        w = self._device_tensor("wavelengths", wavelengths, (n,), missing=TypeError)
        chroma = self._result("chroma", None, (n, 6), samples) if chromatic else None
        self._check(self._lib.zoic_ray_differentials_spectral_device(
            self._h, n, samples.data_ptr(), w.data_ptr(), rs_ptr, int(ray_index_base), rays.data_ptr(), float(dsx), float(dsy),
            out.data_ptr(), chroma.data_ptr() if chromatic else None, self._stream(stream)))
        return (out, chroma) if chromatic else out

    def transmittance(self, samples, rays, wavelengths=None, rng_states=None, ray_index_base=0, out=None, stream=None):
        """Fresnel transmittance (zoic_ray_transmittance_device) of rays create_rays / create_rays_hero made from device tensors: the
        share of unpolarised light the lens's interfaces let through along each record's path, with the coatings of set_coatings.
        Multilayer stacks (set_coating_stacks) are honoured where an interface has one.

        samples, wavelengths, rng_states, ray_index_base: what the forward call was given; rays: the record tensor it returned (or its
        result dict).  wavelengths None: (n,8) records of create_rays(samples), at the d-line; (n,): the spectral records of
        create_rays(samples, wavelengths=); (n,k): the hero records of create_rays_hero, rays (n,k,8).  Returns a float32 device tensor
        of the wavelengths' shape ((n,) for None); asynchronous on `stream` (default: torch's current stream).  Records of weight 0
        and columns whose wavelength is outside [360, 830] or NaN get +0.0.  Changes no record and no counter."""
        n = self._device_tensor("samples", samples, (None, 4)).shape[0]
        shape, w_ptr = (n,), None
        if wavelengths is not None:
            hero = getattr(wavelengths, "ndim", 1) == 2
            shape = tuple(self._device_tensor("wavelengths", wavelengths, (n, None) if hero else (n,), missing=TypeError).shape)
            w_ptr = wavelengths.data_ptr()
        rays, rs_ptr = self._traced(n, rays, rng_states, shape)
        out = self._result("out", out, shape, samples)
        self._check(self._lib.zoic_ray_transmittance_device(self._h, n, shape[1] if len(shape) == 2 else 1, samples.data_ptr(), w_ptr, rs_ptr,
                                                            int(ray_index_base), rays.data_ptr(), out.data_ptr(), self._stream(stream)))
        return out

    def set_coatings(self, index, lambda0_nm):
        """Single-layer coatings in FILE order (front to rear, as the prescription lists the interfaces): the film's index and the
        wavelength (nm) at which it is a quarter wave thick, one per interface (a scalar lambda0_nm serves all); index 0: uncoated.
        set_coatings(None, None) clears them.  An interface with a multilayer stack (set_coating_stacks) is priced by the stack."""
        if index is None:
            self._check(self._lib.zoic_camera_set_coatings(self._h, 0, None, None))
            return
        nc = np.ascontiguousarray(index, dtype=np.float32).reshape(-1)
        l0 = np.ascontiguousarray(np.broadcast_to(np.asarray(lambda0_nm, dtype=np.float32).reshape(-1), nc.shape), dtype=np.float32)
        self._check(self._lib.zoic_camera_set_coatings(self._h, nc.shape[0], nc.ctypes.data, l0.ctypes.data))

    def coatings(self):
        """The lens's film table (zoic_camera_get_coatings), trace order (rear first): dict of float32 arrays index (0: uncoated) and
        lambda0_nm.  Works on a tables-only camera (device=-1)."""
        return self._table(self._lib.zoic_camera_get_coatings, np.float32, ("index", "lambda0_nm"))

    def set_coating_stacks(self, stacks):
        """Multilayer coatings (zoic_camera_set_coating_stacks, csrc/coating_stack.hpp): one entry per interface in FILE order (front
        to rear), each a sequence of up to 8 (index, thickness_nm) pairs, layer 0 adjoining the front-side medium; an empty entry or
        None: no stack there, the interface's set_coatings film (or the bare interface) holds.  set_coating_stacks(None) clears.
        Read at the call: no update is needed."""
        if stacks is None:
            self._check(self._lib.zoic_camera_set_coating_stacks(self._h, 0, None, None, None))
            return
        stacks = list(stacks)
        count, width = len(stacks), _capi.COATING_MAX_LAYERS
        layers = np.zeros(count, np.int32)
        index, thick = np.zeros((count, width), np.float32), np.zeros((count, width), np.float32)
        for i, entry in enumerate(stacks):
            pairs = np.zeros((0, 2), np.float32) if entry is None or len(entry) == 0 else np.asarray(entry, dtype=np.float32)
            if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] > width:
                raise ValueError("stack %d must be a sequence of at most %d (index, thickness_nm) pairs" % (i, width))
            layers[i] = pairs.shape[0]
            index[i, :layers[i]], thick[i, :layers[i]] = pairs[:, 0], pairs[:, 1]
        self._check(self._lib.zoic_camera_set_coating_stacks(self._h, count, layers.ctypes.data, index.ctypes.data, thick.ctypes.data))

    def coating_stacks(self):
        """The lens's stack table (zoic_camera_get_coating_stacks), trace order (rear first), each interface's layers in the order a
        forward ray (rear to front) meets them: dict of layers (count,) int32, index (count,8) and thickness_nm (count,8) float32.
        Works on a tables-only camera (device=-1)."""
        get = self._lib.zoic_camera_get_coating_stacks
        n = get(self._h, 0, None, None, None)
        if n < 0:
            self._check(1)
        width = _capi.COATING_MAX_LAYERS
        a = dict(layers=np.zeros(n, np.int32), index=np.zeros((n, width), np.float32), thickness_nm=np.zeros((n, width), np.float32))
        get(self._h, n, *[v.ctypes.data for v in a.values()])
        return a

    def ghost_pairs(self):
        """The interface pairs that can make a ghost (zoic_camera_get_ghost_pairs): an (m,2) int32 array of rows (a, b), trace-order
        indices (rear first), a > b, both interfaces between unequal media at the d-line; ordered by a, then b.  Works on a
        tables-only camera (device=-1)."""
        packed = self._table(self._lib.zoic_camera_get_ghost_pairs, np.uint32, ("packed",))["packed"]
        return np.stack([packed & _GHOST_INDEX_MASK, (packed >> _GHOST_INDEX_BITS) & _GHOST_INDEX_MASK], 1).astype(np.int32)

    def create_ghost_rays(self, samples, rays, pairs, wavelengths=None, rng_states=None, ray_index_base=0, out=None, stream=None):
        """Ghost rays (zoic_create_ghost_rays_device) of rays create_rays made from device tensors: for every sample and every pair
        (a, b) of `pairs` -- (p,2) integers, trace-order interface indices, a > b: ghost_pairs() lists the ones that reflect -- the
        path that is reflected at a and again at b, with its Fresnel weight (csrc/ghost.hpp).  Multilayer stacks
        (set_coating_stacks) are honoured where an interface has one.

        samples, wavelengths, rng_states, ray_index_base: what the forward call was given; rays: the (n,8) record tensor it returned
        (or its result dict); wavelengths None: the records of create_rays(samples), at the d-line, else the (n,) tensor of
        create_rays(samples, wavelengths=).  Returns an (n,p,8) float32 device tensor of records: origin, dir, weight and the flag
        word (bit 0: traced; else the reason in bits 8-11, the interface in bits 16-21, the leg in bits 24-25 and zeros before
        them).  More than 32 pairs are served by successive calls on the same stream.  out: an optional contiguous (n,p,8) float32
        tensor on the samples' device to write into (p <= 32).  Changes no record and no counter."""
        n = self._device_tensor("samples", samples, (None, 4)).shape[0]
        rays, rs_ptr = self._traced(n, rays, rng_states)
        pr = np.asarray(pairs)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] == 0 or not np.issubdtype(pr.dtype, np.integer):
            raise ValueError("pairs must be a non-empty (p,2) integer array of (a, b)")
        if (pr < 0).any() or (pr > _GHOST_INDEX_MASK).any():
            raise ValueError("pair indices must lie in 0 ... %d" % _GHOST_INDEX_MASK)
        packed = np.ascontiguousarray(pr[:, 0].astype(np.uint32) | (pr[:, 1].astype(np.uint32) << _GHOST_INDEX_BITS))
        w_ptr = self._wavelength_pointer(wavelengths, n)
        p = len(packed)
        chunk = 32   # ZOIC_GHOST_MAX_PAIRS
        if p > chunk and out is not None:
            raise ValueError("out is for at most 32 pairs: more are gathered into a tensor of the call's own")
        if p > chunk and stream is not None:
            raise ValueError("more than 32 pairs are gathered with torch on the current stream: leave stream=None")
        parts = []
        for lo in range(0, p, chunk):   # (one chunk: straight into out)
            q = packed[lo:lo + chunk]
            parts.append(self._result("out", out, (n, len(q), 8), samples))
            self._check(self._lib.zoic_create_ghost_rays_device(self._h, n, len(q), q.ctypes.data, samples.data_ptr(), w_ptr, rs_ptr,
                                                                int(ray_index_base), rays.data_ptr(), parts[-1].data_ptr(), self._stream(stream)))
        if len(parts) == 1:
            return parts[0]
        import torch
        return torch.cat(parts, 1)

    def tile(self, capacity, tid=0):
        """A ZoicTile of this camera (closed with the camera at the latest: ZoicCamera.close() closes the tiles still alive)."""
        return ZoicTile(self, capacity, tid)

    def create_rays_tile(self, inputs, ray_index_base=0, tid=0, out=None):
        """(n,7) float32 AtCameraInput rows -> (n,21) float32 AtCameraOutput rows through the resident kernel
        (zoic_camera_create_rays_tile): page-locked arrays (PinnedArray) are used in place, numpy arrays are staged."""
        a = inputs if (isinstance(inputs, np.ndarray) and inputs.dtype == np.float32 and inputs.flags.c_contiguous) else np.ascontiguousarray(inputs, dtype=np.float32)
        n = a.shape[0]
        outs = out if out is not None else np.empty((n, 21), dtype=np.float32)
        self._check(self._lib.zoic_camera_create_rays_tile(self._h, n, a.ctypes.data_as(C.POINTER(_capi.CameraInput)),
                                                           outs.ctypes.data_as(C.POINTER(_capi.CameraOutput)), int(ray_index_base), int(tid) & 0xFFFF))
        return outs

    def generate_samples(self, n, width, height, spp, seed=1, ray_index_base=0, out=None, stream=None):
        """Synthetic camera samples on the device (torch tensor out)."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        self._check(self._lib.zoic_generate_samples_device(self._h, n, int(ray_index_base), width, height, spp, seed,
                                                           out.data_ptr(), self._stream(stream)))
        return out

    # ------------------------------------------------------------------ statistics / tables
    def counters(self):
        c = _capi.Counters()
        self._check(self._lib.zoic_camera_get_counters(self._h, C.byref(c)))
        return dict(succesRays=c.succesRays, vignettedRays=c.vignettedRays, totalInternalReflection=c.totalInternalReflection)

    def reset_counters(self):
        self._check(self._lib.zoic_camera_reset_counters(self._h))

    def info(self):
        i = _capi.LensInfo()
        self._check(self._lib.zoic_camera_get_info(self._h, C.byref(i)))
        n = i.lensCount
        f = lambda a, m: np.array(a[:m], dtype=np.float32)  # noqa: E731
        elements = np.stack([f(i.curvature, n), f(i.thickness, n), f(i.ior, n), f(i.aperture, n), f(i.center, n)], 1) \
            if n else np.zeros((0, 5), np.float32)
        return dict(lensCount=n, apertureElement=i.apertureElement, elements=elements,
                    userApertureRadius=np.float32(i.userApertureRadius), originShift=np.float32(i.originShift),
                    apertureDistance=np.float32(i.apertureDistance), focalLengthRatio=np.float32(i.focalLengthRatio),
                    tracedFocalLength=(np.float32(i.tracedFocalLength[0]), np.float32(i.tracedFocalLength[1])),
                    fov=np.float32(i.fov), tan_fov=np.float32(i.tan_fov), apertureRadius=np.float32(i.apertureRadius),
                    lutKeys=f(i.lutKey, i.lutSize),
                    lutBoxes=np.stack([f(i.lutMaxX, i.lutSize), f(i.lutMaxY, i.lutSize), f(i.lutMinX, i.lutSize),
                                       f(i.lutMinY, i.lutSize)], 1),
                    bokehWidth=i.bokehWidth, bokehHeight=i.bokehHeight, fastRunsStrict=bool(i.fastRunsStrict), precomputeTIR=int(i.precomputeTIR))

    def bokeh_tables(self):
        i = self.info()
        x, y = i["bokehWidth"], i["bokehHeight"]
        if x <= 0 or y <= 0:
            return None
        t = dict(x=x, y=y, cdfRow=np.empty(y, np.float32), rowIndices=np.empty(y, np.int32),
                 cdfColumn=np.empty(x * y, np.float32), columnIndices=np.empty(x * y, np.int32))
        self._check(self._lib.zoic_camera_get_bokeh_tables(self._h, t["cdfRow"].ctypes.data, t["rowIndices"].ctypes.data,
                                                           t["cdfColumn"].ctypes.data, t["columnIndices"].ctypes.data))
        return t

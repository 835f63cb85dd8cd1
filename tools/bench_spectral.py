#!/usr/bin/env python3
"""Cost of rays at a wavelength per ray (zoic_create_rays_spectral_device) against the plain ray call on the same samples: C2 (TESSAR,
the prescription's V-numbers), C5 (PETZVAL, the prescription's V-numbers) and C3 (DOUBLE_GAUSS + bokeh image, which ships no
V-numbers: a SYNTHETIC V = 50 on every glass), in FAST and STRICT, one JSON line.

    python tools/bench_spectral.py [--reps 3] [--configs C2,C3,C5] [--precisions fast,strict] [--max-rays 67108864]

Per config the first min(frame, --max-rays) rays of the frame run in slabs of at most 2^26 rays; every slab's samples are synthesised on
the device, and so are its wavelengths: uniform in [400, 700] nm from a seeded hash of the ray index.  The plain and the spectral call
are timed with device events on one stream, after one warm-up frame; plain_ms / spectral_ms: the mean over --reps frames.  Kernel
times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLAB = 1 << 26
SYNTHETIC_V = 50.0


def wavelengths(torch, base, m, out, seed=0x5eed):
    """uniform in [400, 700) nm from a 32-bit hash of (seed, ray index), computed on the device"""
    mask = 0xFFFFFFFF
    h = (torch.arange(base, base + m, dtype=torch.int64, device=out.device) ^ seed) & mask
    for mul in (0x7FEB352D, 0x846CA68B):   # lowbias32
        h = (h ^ (h >> 16)) & mask
        h = (h * mul) & mask
    h = h ^ (h >> 16)
    out[:m] = 400.0 + 300.0 * ((h >> 8).to(torch.float32) * (1.0 / 16777216.0))
    return out[:m]


def frame(torch, cam, c, n, bufs, stream, timed):
    s, lam, rays = bufs
    plain = spec = 0.0
    for base in range(0, n, SLAB):
        m = min(SLAB, n - base)
        cam.generate_samples(m, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base, out=s[:m], stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            w = wavelengths(torch, base, m, lam)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(stream)
        cam.create_rays(s[:m], ray_index_base=base, out=dict(rays=rays[:m]), stream=stream.cuda_stream)
        e[1].record(stream)
        cam.create_rays(s[:m], ray_index_base=base, out=dict(rays=rays[:m]), stream=stream.cuda_stream, wavelengths=w)
        e[2].record(stream)
        e[2].synchronize()
        if timed:
            plain += e[0].elapsed_time(e[1])
            spec += e[1].elapsed_time(e[2])
    return plain, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="C2,C5,C3")
    ap.add_argument("--precisions", default="fast,strict")
    ap.add_argument("--max-rays", type=int, default=1 << 26)
    a = ap.parse_args()
    import torch
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_spectral: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_spectral", "wavelengths_nm": [400, 700], "configs": []}
    for cfg in a.configs.split(","):
        c = CONFIGS[cfg]
        n = min(c["width"] * c["height"] * c["spp"], a.max_rays)
        m = min(n, SLAB)
        bufs = (torch.empty((m, 4), dtype=torch.float32, device=dev), torch.empty((m,), dtype=torch.float32, device=dev),
                torch.empty((m, 8), dtype=torch.float32, device=dev))
        for prec in a.precisions.split(","):
            cam = ZoicCamera(device=0)
            if c["bokeh"]:
                cam.set_bokeh_image(hexagon_bokeh())
            cam.set_precision(PRECISION_FAST if prec == "fast" else PRECISION_STRICT)
            p = camera_params(cfg)
            glass = "file"
            if cfg == "C3":
                count = ZoicCamera(device=-1).update(**dict(p, useImage=False)).info()["lensCount"]
                cam.set_abbe_numbers([SYNTHETIC_V] * count)
                glass = "synthetic V=%g" % SYNTHETIC_V
            cam.update(**p)
            frame(torch, cam, c, n, bufs, stream, False)
            plain = spec = 0.0
            for _ in range(a.reps):
                pl, sp = frame(torch, cam, c, n, bufs, stream, True)
                plain += pl / a.reps
                spec += sp / a.reps
            result["configs"].append({"config": cfg, "precision": prec, "abbe": glass, "rays": n,
                                      "fast_runs_strict": bool(cam.info()["fastRunsStrict"]),
                                      "plain_ms": round(plain, 3), "spectral_ms": round(spec, 3), "spectral_over_plain": round(spec / plain, 3),
                                      "spectral_grays_per_s": round(n / spec / 1e6, 2)})
            cam.close()
        del bufs
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

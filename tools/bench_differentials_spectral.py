#!/usr/bin/env python3
"""Cost of the traced ray differentials of spectral records (zoic_ray_differentials_spectral_device) against the d-line differential
pass (zoic_ray_differentials_device) over the same records: C2, C3 (V = 50 for every glass) and C5, one JSON line.

    python tools/bench_differentials_spectral.py [--reps 3] [--precision fast|strict] [--max-rays N]

Per config the frame (or its first --max-rays rays) runs in slabs of at most 2^27 rays; every slab's samples are synthesised on the
device, its wavelengths are uniform in [400, 700] nm, the spectral ray pass writes the records, and three passes over those records
are timed with device events on one stream, after one warm-up frame:
    dline_ms      zoic_ray_differentials_device (the d-line tangents: not valid for these records, the yardstick for the cost)
    spectral_ms   zoic_ray_differentials_spectral_device without d_chromatic (12 floats)
    chromatic_ms  the same call with d_chromatic (12 + 6 floats)
Each is the mean over --reps frames.  Per ray the spectral passes read 4 B more (the wavelength) and the chromatic one writes 24 B
more.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLAB = 1 << 27
ABBE = {"C3": 50.0}   # the double Gauss ships no V-numbers


def frame(torch, cam, c, n, bufs, stream, timed):
    """one frame in slabs: (d-line ms, spectral ms, chromatic ms) by device events"""
    s, lam, rays, out, chroma = bufs
    ms = [0.0, 0.0, 0.0]
    for base in range(0, n, SLAB):
        m = min(SLAB, n - base)
        st = stream.cuda_stream
        cam.generate_samples(m, c["width"], c["height"], c["spp"], seed=1, ray_index_base=base, out=s[:m], stream=st)
        cam.create_rays(s[:m], ray_index_base=base, out=dict(rays=rays[:m]), stream=st, wavelengths=lam[:m])
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        cam.ray_differentials(s[:m], rays[:m], ray_index_base=base, out=out[:m], stream=st)
        e[1].record(stream)
        cam.ray_differentials(s[:m], rays[:m], ray_index_base=base, out=out[:m], stream=st, wavelengths=lam[:m])
        e[2].record(stream)
        # (ZoicCamera.ray_differentials allocates the chromatic tensor per call: the C call keeps the allocation out of the timing)
        cam._check(cam._lib.zoic_ray_differentials_spectral_device(cam._h, m, s.data_ptr(), lam.data_ptr(), None, base, rays.data_ptr(), 1.0, 1.0,
                                                                   out.data_ptr(), chroma.data_ptr(), st))
        e[3].record(stream)
        e[3].synchronize()
        if timed:
            for k in range(3):
                ms[k] += e[k].elapsed_time(e[k + 1])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--max-rays", type=int, default=0, help="cap on the rays per config (0: the whole frame)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_differentials_spectral: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_differentials_spectral", "precision": a.precision, "wavelengths_nm": [400, 700], "configs": []}
    for cfg in a.configs.split(","):
        c = CONFIGS[cfg]
        n = c["width"] * c["height"] * c["spp"]
        if a.max_rays > 0:
            n = min(n, a.max_rays)
        cam = ZoicCamera(device=0)
        if c["bokeh"]:
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_FAST if a.precision == "fast" else PRECISION_STRICT)
        cam.update(**camera_params(cfg))
        if cfg in ABBE:
            cam.set_abbe_numbers(np.full(cam.info()["lensCount"], ABBE[cfg], np.float32))
        m = min(n, SLAB)
        g = torch.Generator(device=dev)
        g.manual_seed(4)
        lam = torch.empty(m, dtype=torch.float32, device=dev).uniform_(400.0, 700.0, generator=g)
        bufs = (torch.empty((m, 4), dtype=torch.float32, device=dev), lam, torch.empty((m, 8), dtype=torch.float32, device=dev),
                torch.empty((m, 12), dtype=torch.float32, device=dev), torch.empty((m, 6), dtype=torch.float32, device=dev))
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            frame(torch, cam, c, n, bufs, stream, False)
            ms = [0.0, 0.0, 0.0]
            for _ in range(a.reps):
                for k, v in enumerate(frame(torch, cam, c, n, bufs, stream, True)):
                    ms[k] += v / a.reps
        live = float((bufs[2][:m, 6] != 0).float().mean())
        result["configs"].append({"config": cfg, "rays": n, "dline_ms": round(ms[0], 3), "spectral_ms": round(ms[1], 3),
                                  "chromatic_ms": round(ms[2], 3), "spectral_over_dline": round(ms[1] / ms[0], 3),
                                  "chromatic_over_dline": round(ms[2] / ms[0], 3), "live_frac_last_slab": round(live, 4)})
        del bufs, lam
        torch.cuda.empty_cache()
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the Fresnel transmittance pass (zoic_ray_transmittance_device) over hero records with k = 1, 4 and 8 wavelengths per
sample, beside the spectral differential pass (zoic_ray_differentials_spectral_device without d_chromatic) over the same samples'
k = 1 records: C2 and C3 (V = 50 for every glass), one JSON line.

    python tools/bench_transmittance.py [--reps 3] [--precision fast|strict] [--max-rays N]

Per config the frame's first --max-rays samples are synthesised on the device; the wavelengths are uniform in [400, 700] nm.  For each k
the hero call writes the n x k records, then two passes over them are timed with device events on one stream, after one warm-up:
    bare_ms   the transmittance pass, no coating
    film_ms   the same with a 1.38-index film, a quarter wave thick at 550 nm, on every interface
and on the k = 1 records
    diff_ms   zoic_ray_differentials_spectral_device, 12 floats (a primal and two tangents per record)
Each is the mean over --reps runs; *_ns_per_column divides by the n k columns (live or not).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ABBE = {"C3": 50.0}   # the double Gauss ships no V-numbers
KS = (1, 4, 8)


def timed(torch, stream, reps, call):
    """mean ms of call() over reps runs by device events, after one warm-up"""
    call()
    total = 0.0
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        total += a.elapsed_time(b)
    return total / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--max-rays", type=int, default=1 << 22, help="cap on the samples per config (0: the whole frame)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_transmittance: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_transmittance", "precision": a.precision, "wavelengths_nm": [400, 700], "film": [1.38, 550.0], "configs": []}
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
        count = cam.info()["lensCount"]
        if cfg in ABBE:
            cam.set_abbe_numbers(np.full(count, ABBE[cfg], np.float32))
        film = np.full(count, 1.38, np.float32)
        g = torch.Generator(device=dev)
        g.manual_seed(4)
        st = stream.cuda_stream
        row = {"config": cfg, "samples": n, "k": {}}
        with torch.cuda.stream(stream):
            s = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1, stream=st)
            for k in KS:
                lam = torch.empty((n, k), dtype=torch.float32, device=dev).uniform_(400.0, 700.0, generator=g)
                rays = cam.create_rays_hero(s, lam, stream=st)["rays"]
                out = torch.empty((n, k), dtype=torch.float32, device=dev)
                run = lambda: cam.transmittance(s, rays, wavelengths=lam, out=out, stream=st)   # noqa: E731
                cam.set_coatings(None, None)
                bare = timed(torch, stream, a.reps, run)
                cam.set_coatings(film, 550.0)
                coated = timed(torch, stream, a.reps, run)
                live = rays[:, :, 6] != 0
                r = {"bare_ms": round(bare, 3), "film_ms": round(coated, 3), "bare_ns_per_column": round(bare * 1e6 / (n * k), 3),
                     "film_ns_per_column": round(coated * 1e6 / (n * k), 3), "live_frac": round(float(live.float().mean()), 4),
                     "median_T_film": round(float(out[live].median()), 4)}
                if k == 1:
                    d = torch.empty((n, 12), dtype=torch.float32, device=dev)
                    r1, l1 = rays.view(n, 8), lam.view(n)
                    ms = timed(torch, stream, a.reps, lambda: cam.ray_differentials(s, r1, out=d, stream=st, wavelengths=l1))
                    row["diff_ms"], row["diff_ns_per_column"] = round(ms, 3), round(ms * 1e6 / n, 3)
                    del d
                row["k"][str(k)] = r
                del lam, rays, out
                torch.cuda.empty_cache()
        result["configs"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

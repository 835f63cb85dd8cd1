#!/usr/bin/env python3
"""Cost of hero-wavelength rays (zoic_create_rays_hero_device) against the existing way to get k wavelengths per sample -- k calls of
zoic_create_rays_spectral_device on the same samples -- and against one such call: C2 (TESSAR, the prescription's V-numbers), C5
(PETZVAL, the prescription's V-numbers) and C3 (DOUBLE_GAUSS + bokeh image with a SYNTHETIC V = 50 on every glass), in FAST and STRICT,
k in {1, 4, 8}, one JSON line.

    python tools/bench_hero.py [--reps 3] [--configs C2,C5,C3] [--precisions fast,strict] [--ks 1,4,8] [--max-rays 16777216]

Per config the first min(frame, --max-rays) samples of the frame are synthesised on the device, and so are their wavelengths: uniform
in [400, 700] nm from a seeded hash of (sample, column), the hero in column 0.  The three legs are timed with device events on one
stream, after one warm-up frame; hero_ms / k_calls_ms / one_call_ms: the mean over --reps frames.  k_calls_ms runs the spectral call
once per column on that column's wavelengths; one_call_ms is its first call (k = 1: hero_ms must be within noise of it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_spectral import SYNTHETIC_V, wavelengths  # noqa: E402


def frame(torch, cam, n, k, bufs, stream):
    """(hero, k calls, first of the k calls) in ms"""
    s, lam, cols, rays, one = bufs
    e = [torch.cuda.Event(enable_timing=True) for _ in range(k + 2)]
    e[0].record(stream)
    cam.create_rays_hero(s, lam, out=dict(rays=rays[:n * k].view(n, k, 8)), stream=stream.cuda_stream)
    e[1].record(stream)
    for j in range(k):
        cam.create_rays(s, out=dict(rays=one), stream=stream.cuda_stream, wavelengths=cols[j])
        e[2 + j].record(stream)
    e[-1].synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[-1]), e[1].elapsed_time(e[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="C2,C5,C3")
    ap.add_argument("--precisions", default="fast,strict")
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--max-rays", type=int, default=1 << 24)
    a = ap.parse_args()
    import torch
    from zoic_amd import HERO_MAX_WAVELENGTHS, PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_hero: no GPU visible (nothing measured)")
    ks = [int(x) for x in a.ks.split(",")]
    kmax = max(ks)
    assert 1 <= min(ks) and kmax <= HERO_MAX_WAVELENGTHS
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_hero", "wavelengths_nm": [400, 700], "configs": []}
    for cfg in a.configs.split(","):
        c = CONFIGS[cfg]
        n = min(c["width"] * c["height"] * c["spp"], a.max_rays)
        s = torch.empty((n, 4), dtype=torch.float32, device=dev)
        cols = torch.empty((kmax, n), dtype=torch.float32, device=dev)      # column-major: what the k separate calls read
        rays = torch.empty((n * kmax, 8), dtype=torch.float32, device=dev)
        one = torch.empty((n, 8), dtype=torch.float32, device=dev)
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
            cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1, ray_index_base=0, out=s, stream=stream.cuda_stream)
            with torch.cuda.stream(stream):
                for j in range(kmax):
                    wavelengths(torch, 0, n, cols[j], seed=0x5eed + 977 * j)
            for k in ks:
                with torch.cuda.stream(stream):
                    lam = cols[:k].t().contiguous()                         # sample-major (n, k): what the hero call reads
                bufs = (s, lam, cols, rays, one)
                frame(torch, cam, n, k, bufs, stream)
                hero = calls = first = 0.0
                for _ in range(a.reps):
                    h, kc, f = frame(torch, cam, n, k, bufs, stream)
                    hero += h / a.reps
                    calls += kc / a.reps
                    first += f / a.reps
                result["configs"].append({"config": cfg, "precision": prec, "abbe": glass, "samples": n, "k": k,
                                          "fast_runs_strict": bool(cam.info()["fastRunsStrict"]),
                                          "hero_ms": round(hero, 3), "k_calls_ms": round(calls, 3), "one_call_ms": round(first, 3),
                                          "hero_over_k_calls": round(hero / calls, 3), "hero_over_one_call": round(hero / first, 3),
                                          "hero_grecords_per_s": round(n * k / hero / 1e6, 2)})
                del lam
            cam.close()
        del s, cols, rays, one
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

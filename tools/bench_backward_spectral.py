#!/usr/bin/env python3
"""Rate of the two backward calls at a wavelength per item next to their d-line siblings on the same items, one JSON line.

    python tools/bench_backward_spectral.py [--reps 5] [--width 3840 --height 2160 --spp 2]

Per camera (C2 TESSAR with its file's V-numbers, C3 DOUBLE_GAUSS with a synthetic V = 50 for every glass as tools/bench_spectral.py
uses, C5 PETZVAL with its file's, and the thin lens of C1; STRICT): the forward records of a full frame of synthetic samples
(zoic_create_rays_device) are traced back by zoic_trace_back_rays_device and by zoic_trace_back_rays_spectral_device, and one point
per record (its origin moved focalDistance along its direction) is projected by zoic_project_points_device and by
zoic_project_points_spectral_device; wavelengths uniform in [400, 700] nm.  In one run, on one stream, every call timed with device
events after one warm-up, mean over --reps calls.  The spectral trace-back moves 48 B per ray (32 + 4 in, 8 + 4 out) against 44, the
spectral projection 28 B per point against 24.  ratio = spectral ms / d-line ms.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_backward_spectral: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = a.width * a.height * a.spp
    smp = torch.empty((n, 4), dtype=torch.float32, device=dev)
    lam = torch.empty((n,), dtype=torch.float32, device=dev).uniform_(400.0, 700.0)

    def timed(fn):
        torch.cuda.synchronize(dev)
        fn()   # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    result = {"tool": "bench_backward_spectral", "frame": [a.width, a.height, a.spp], "items": n, "cameras": []}
    for name, cfg, abbe in (("C2", "C2", None), ("C3", "C3", 50.0), ("C5", "C5", None), ("thin", "C1", None)):
        p = camera_params(cfg)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_STRICT)
        cam.update(**p)
        if abbe is not None:
            cam.set_abbe_numbers(np.full(cam.info()["lensCount"], abbe, np.float32))
        st = cam._lib.zoic_generate_samples_device(cam._h, n, 0, a.width, a.height, a.spp, 1, smp.data_ptr(), None)
        assert st == 0, st
        torch.cuda.synchronize(dev)
        rays = cam.create_rays(smp)["rays"]
        d = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True).clamp_min(1e-30)
        pts = (rays[:, 0:3] + d * float(p["focalDistance"])).contiguous()
        del d
        scr = torch.empty((n, 2), dtype=torch.float32, device=dev)
        fl = torch.empty((n,), dtype=torch.int32, device=dev)
        row = {"camera": name, "lens": os.path.basename(p.get("lensDataPath") or "thin"), "abbe": "file" if abbe is None else abbe}
        for label, call, items, unit, nbytes in (("trace_back", cam.trace_back, rays, "Grays_per_s", 44),
                                                 ("project_points", cam.project_points, pts, "Gpoints_per_s", 24)):
            ms_d = timed(lambda: call(items, out=scr, flags=fl, stream=stream.cuda_stream))
            done_d = float(((fl & 1) != 0).float().mean().item())
            ms_s = timed(lambda: call(items, out=scr, flags=fl, stream=stream.cuda_stream, wavelengths=lam))
            done_s = float(((fl & 1) != 0).float().mean().item())
            row[label] = {"d_line": {"ms": round(ms_d, 4), unit: round(n / ms_d / 1e6, 3), "GB_per_s": round(n * nbytes / ms_d / 1e6, 1),
                                     "done": round(done_d, 5)},
                          "spectral": {"ms": round(ms_s, 4), unit: round(n / ms_s / 1e6, 3), "GB_per_s": round(n * (nbytes + 4) / ms_s / 1e6, 1),
                                       "done": round(done_s, 5)},
                          "ratio": round(ms_s / ms_d, 3)}
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

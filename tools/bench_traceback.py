#!/usr/bin/env python3
"""Rate of the trace-back (zoic_trace_back_rays_device) next to the forward frame that made its input and to the reverse projection
on as many points, one JSON line.

    python tools/bench_traceback.py [--reps 5] [--width 3840 --height 2160 --spp 2]

Per camera (C2 TESSAR, C3 DOUBLE_GAUSS, C5 PETZVAL and the thin lens of C1, STRICT): the forward records of a full frame of
synthetic samples (zoic_create_rays_device) are traced back twice, all of them and the compacted ones of weight > 0.  In the same run,
on the same stream: the forward call itself, and zoic_project_points_device on one point per record (the record's origin moved
focalDistance along its direction).  Every call is timed with device events after one warm-up, mean over --reps calls.  The
trace-back moves 44 B per ray (32 in, 8 + 4 out): bytes/s is that times rays/s.  traced: the share of the rays with flag bit 0.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_RAY = 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=2)
    a = ap.parse_args()
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_traceback: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = a.width * a.height * a.spp
    smp = torch.empty((n, 4), dtype=torch.float32, device=dev)

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

    result = {"tool": "bench_traceback", "frame": [a.width, a.height, a.spp], "rays": n, "cameras": []}
    for name, cfg in (("C2", "C2"), ("C3", "C3"), ("C5", "C5"), ("thin", "C1")):
        p = camera_params(cfg)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_STRICT)
        cam.update(**p)
        st = cam._lib.zoic_generate_samples_device(cam._h, n, 0, a.width, a.height, a.spp, 1, smp.data_ptr(), None)
        assert st == 0, st
        torch.cuda.synchronize(dev)
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        fwd_ms = timed(lambda: cam.create_rays(smp, out=dict(rays=rays), stream=stream.cuda_stream))
        row = {"camera": name, "lens": os.path.basename(p.get("lensDataPath") or "thin"),
               "forward": {"ms": round(fwd_ms, 4), "Grays_per_s": round(n / fwd_ms / 1e6, 3)}}
        live = rays[rays[:, 6] > 0].contiguous()
        for label, r in (("all", rays), ("live", live)):
            m = r.shape[0]
            scr = torch.empty((m, 2), dtype=torch.float32, device=dev)
            fl = torch.empty((m,), dtype=torch.int32, device=dev)
            ms = timed(lambda: cam.trace_back(r, out=scr, flags=fl, stream=stream.cuda_stream))
            row["trace_back_" + label] = {"rays": m, "ms": round(ms, 4), "Grays_per_s": round(m / ms / 1e6, 3),
                                          "GB_per_s": round(m * BYTES_PER_RAY / ms / 1e6, 1),
                                          "traced": round(float(((fl & 1) != 0).float().mean().item()), 5)}
        d = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True).clamp_min(1e-30)
        pts = (rays[:, 0:3] + d * float(p["focalDistance"])).contiguous()
        scr = torch.empty((n, 2), dtype=torch.float32, device=dev)
        fl = torch.empty((n,), dtype=torch.int32, device=dev)
        ms = timed(lambda: cam.project_points(pts, out=scr, flags=fl, stream=stream.cuda_stream))
        row["project_points"] = {"points": n, "ms": round(ms, 4), "Gpoints_per_s": round(n / ms / 1e6, 3),
                                 "projected": round(float(((fl & 1) != 0).float().mean().item()), 5)}
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

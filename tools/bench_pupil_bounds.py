#!/usr/bin/env python3
"""Rate of the pupil bounds (zoic_pupil_bounds_device) next to the trace-back of the same rays given explicitly, one JSON line.

    python tools/bench_pupil_bounds.py [--reps 5] [--points 32768]

Per camera (C3 DOUBLE_GAUSS wide open and at f/8, C5 PETZVAL, the thin lens of C1) and lattice size G (8, 16, 32): --points scene
points spread over the field at 20 ... 1000 cm are bounded in one call; the yardstick is zoic_trace_back_rays_device on the same
points x G^2 rays written out as zoic_ray records (origin = P, dir = P - aim), in the same run on the same stream.  The bounds move
12 + 48 bytes per point, the explicit rays 44 bytes per aim.  Every call is timed with device events after one warm-up, mean over
--reps calls.  ratio: aims/s of the bounds over rays/s of the trace-back (> 1: the bounds are faster per aim).  passing: the share
of aims that pass; the same share of the explicit rays is traced back, which the tool checks.
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
    ap.add_argument("--points", type=int, default=32768)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_pupil_bounds: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = a.points

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

    result = {"tool": "bench_pupil_bounds", "points": n, "cameras": []}
    rng = np.random.default_rng(1)
    for name, cfg, over in (("C3", "C3", {}), ("C3-f8", "C3", dict(fStop=8.0)), ("C5", "C5", {}), ("thin", "C1", {})):
        p = dict(camera_params(cfg), **over)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.update(**p)
        field = 0.5 * float(p["sensorWidth"]) / float(p["focalLength"])
        depth = 10.0 ** rng.uniform(np.log10(20.0), 3.0, n)
        pts_h = np.stack([rng.uniform(-0.8, 0.8, n) * field * depth, rng.uniform(-0.5, 0.5, n) * field * depth, -depth], 1).astype(np.float32)
        pts = torch.from_numpy(pts_h).to(dev)
        z, R = cam.pupil_square()
        row = {"camera": name, "lens": os.path.basename(p.get("lensDataPath") or "thin"), "lattices": []}
        for G in (8, 16, 32):
            out = torch.empty((n, 12), dtype=torch.float32, device=dev)
            ms = timed(lambda: cam.pupil_bounds(pts, G, out=out, stream=stream.cuda_stream))
            count = out[:, 8].view(torch.int32).sum().item()
            # the same rays, explicit: aims in the definition's f32 operations
            c = (torch.arange(G, device=dev, dtype=torch.float32) * 2 + (1 - G)) * (np.float32(R) / np.float32(G))
            aims = torch.stack([c.repeat(G), c.repeat_interleave(G), torch.full((G * G,), float(z), device=dev)], 1)
            rays = torch.zeros((n, G * G, 8), dtype=torch.float32, device=dev)
            rays[:, :, 0:3] = pts[:, None, :]
            rays[:, :, 3:6] = pts[:, None, :] - aims[None]
            rays = rays.reshape(-1, 8)
            m = rays.shape[0]
            scr = torch.empty((m, 2), dtype=torch.float32, device=dev)
            fl = torch.empty((m,), dtype=torch.int32, device=dev)
            tb_ms = timed(lambda: cam.trace_back(rays, out=scr, flags=fl, stream=stream.cuda_stream))
            traced = int((fl & 1).sum().item())
            assert traced == count, (name, G, traced, count)
            row["lattices"].append({"G": G, "ms": round(ms, 4), "Mpoints_per_s": round(n / ms / 1e3, 3), "Gaims_per_s": round(m / ms / 1e6, 3),
                                    "passing": round(count / m, 5),
                                    "trace_back": {"rays": m, "ms": round(tb_ms, 4), "Grays_per_s": round(m / tb_ms / 1e6, 3)},
                                    "ratio": round(tb_ms / ms, 3)})
            del rays, scr, fl, out
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of the lens splats (zoic_splat_points_device) next to the trace-back Jacobian of the same rays given explicitly, one JSON line.

    python tools/bench_splats.py [--reps 5] [--points 32768]

Per camera (C3 DOUBLE_GAUSS wide open and at f/8, C5 PETZVAL, the thin lens of C1) and m (16 and 64 aims per point): --points scene
points spread over the field at 20 ... 1000 cm, as tools/bench_pupil_bounds.py places them, are bounded once at lattice 16 and then
splatted in one call with u uniform.  The yardstick is zoic_trace_back_jacobian_device on the same n m rays written out beforehand as
zoic_ray records (origin = P, dir = P - aim, the aims taken from the splat records), in the same run on the same stream: the existing
chain without its host step.  The splats move 8 + 32 bytes per splat and 44 (spectral: 48) per point; the yardstick reads 32 and
writes 8 + 4 + 48 bytes per ray.  Every call is timed with device events after one warm-up, mean over --reps calls.  ratio:
splats/s over rays/s of the yardstick (> 1: the fused call is faster per ray).  The tool checks that both give the same sx, sy and
flags for every ray that has a box.  A single run; the buffers are re-read on every repetition.
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
    from zoic_amd import ZoicCamera, _capi
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_splats: no GPU visible (nothing measured)")
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

    result = {"tool": "bench_splats", "points": n, "lattice": 16, "cameras": []}
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
        z, _ = cam.pupil_square()
        with torch.cuda.stream(stream):
            bounds = cam.pupil_bounds(pts, 16)
        stream.synchronize()
        row = {"camera": name, "lens": os.path.basename(p.get("lensDataPath") or "thin"), "aims": []}
        for m in (16, 64):
            u = torch.from_numpy(rng.random((n, m, 2), dtype=np.float32)).to(dev)
            out = torch.empty((n, m, 8), dtype=torch.float32, device=dev)
            ms = timed(lambda: cam.splat_points(pts, bounds, u, out=out, stream=stream.cuda_stream))
            rec = out.reshape(-1, 8)
            flags = rec[:, 6].view(torch.int32)
            box = (flags & _capi.SPLAT_NO_BOX) == 0
            # the same rays, explicit: dir = P - aim in three f32 subtractions
            k = n * m
            rays = torch.zeros((n, m, 8), dtype=torch.float32, device=dev)
            rays[:, :, 0:3] = pts[:, None, :]
            rays[:, :, 3:5] = pts[:, None, 0:2] - out[:, :, 2:4]
            rays[:, :, 5] = pts[:, None, 2] - torch.tensor(z, dtype=torch.float32, device=dev)
            rays = rays.reshape(-1, 8)
            scr = torch.empty((k, 2), dtype=torch.float32, device=dev)
            fl = torch.empty((k,), dtype=torch.int32, device=dev)
            jac = torch.empty((k, 2, 6), dtype=torch.float32, device=dev)
            tb_ms = timed(lambda: cam.trace_back_jacobian(rays, out=scr, flags=fl, jacobian=jac, stream=stream.cuda_stream))
            same = bool((fl[box] == flags[box]).all().item()) and bool((scr[box].view(torch.int32) == rec[box][:, 0:2].view(torch.int32)).all().item())
            assert same, (name, m)
            traced = int((flags[box] & 1).sum().item())
            row["aims"].append({"m": m, "splats": k, "ms": round(ms, 4), "Gsplats_per_s": round(k / ms / 1e6, 3),
                                "bytes_per_splat": round(40 + 44 / m, 2), "with_box": round(float(box.float().mean().item()), 5),
                                "traced": round(traced / k, 5),
                                "trace_back_jacobian": {"rays": k, "ms": round(tb_ms, 4), "Grays_per_s": round(k / tb_ms / 1e6, 3), "bytes_per_ray": 92},
                                "ratio": round(tb_ms / ms, 3), "same_sx_sy_flags": same})
            del rays, scr, fl, jac, out, u
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

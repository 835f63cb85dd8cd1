#!/usr/bin/env python3
"""Cost of the trace-back Jacobian (zoic_trace_back_jacobian_device and its spectral form) next to the trace-back of the same rays and
to the 13 trace-back calls a central-difference Jacobian needs, one JSON line.

    python tools/bench_traceback_jacobian.py [--reps 5] [--width 1920 --height 1080 --spp 2]

Per camera (C2 TESSAR, C3 DOUBLE_GAUSS, C5 PETZVAL, STRICT), at the d-line and at a wavelength per ray (uniform in 400 ... 700 nm): the
forward records of weight > 0 of a frame of synthetic samples, moved one front housing radius out along the ray (so that the
finite-difference neighbours exist: a record's own origin lies on the front element's cap), are given to
    trace_back            zoic_trace_back_rays_device               44 B per ray (spectral 48)
    jacobian              zoic_trace_back_jacobian_device           92 B per ray (spectral 96)
    finite_differences    the 13 zoic_trace_back_rays_device calls of a central difference (the ray and its 12 neighbours, the
                          neighbour records made beforehand and not timed, the differencing itself not timed either)
Every figure is timed with device events on one stream after one warm-up, mean over --reps.  No ratio is asserted.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP = 2.0 ** -9   # of the front housing radius (origin) and of |dir| = 1 (dir)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=2)
    a = ap.parse_args()
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_traceback_jacobian: no GPU visible (nothing measured)")
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

    result = {"tool": "bench_traceback_jacobian", "frame": [a.width, a.height, a.spp], "cameras": []}
    for cfg in ("C2", "C3", "C5"):
        p = camera_params(cfg)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_STRICT)
        cam.update(**p)
        st = cam._lib.zoic_generate_samples_device(cam._h, n, 0, a.width, a.height, a.spp, 1, smp.data_ptr(), None)
        assert st == 0, st
        rays = cam.create_rays(smp)["rays"]
        torch.cuda.synchronize(dev)
        rays = rays[rays[:, 6] > 0].contiguous()
        m = rays.shape[0]
        info = cam.info()
        radius = float(info["elements"][int(info["lensCount"]) - 1, 3]) * 0.5
        d = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True)
        rays[:, 3:6] = d
        rays[:, 0:3] += radius * d
        neighbours = []
        for col in range(6):
            for sign in (1.0, -1.0):
                r = rays.clone()
                r[:, col] += sign * STEP * (radius if col < 3 else 1.0)
                neighbours.append(r)
        lam = torch.empty((m,), dtype=torch.float32, device=dev).uniform_(400.0, 700.0)
        scr = torch.empty((m, 2), dtype=torch.float32, device=dev)
        fl = torch.empty((m,), dtype=torch.int32, device=dev)
        jac = torch.empty((m, 2, 6), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        row = {"camera": cfg, "lens": os.path.basename(p.get("lensDataPath") or "thin"), "rays": m}
        for label, w, b_tb, b_j in (("d_line", None, 44, 92), ("spectral", lam, 48, 96)):
            def fd():
                for r in [rays] + neighbours:
                    cam.trace_back(r, out=scr, flags=fl, stream=stream.cuda_stream, wavelengths=w)
            tb = timed(lambda: cam.trace_back(rays, out=scr, flags=fl, stream=stream.cuda_stream, wavelengths=w))
            tj = timed(lambda: cam.trace_back_jacobian(rays, wavelengths=w, out=scr, flags=fl, jacobian=jac, stream=stream.cuda_stream))
            traced = round(float(((fl & 1) != 0).float().mean().item()), 5)
            tf = timed(fd)
            row[label] = {"trace_back": {"ms": round(tb, 4), "Grays_per_s": round(m / tb / 1e6, 3), "GB_per_s": round(m * b_tb / tb / 1e6, 1)},
                          "jacobian": {"ms": round(tj, 4), "Grays_per_s": round(m / tj / 1e6, 3), "GB_per_s": round(m * b_j / tj / 1e6, 1),
                                       "traced": traced},
                          "finite_differences": {"ms": round(tf, 4), "Grays_per_s": round(m / tf / 1e6, 3)},
                          "jacobian_over_trace_back": round(tj / tb, 3), "finite_differences_over_jacobian": round(tf / tj, 3)}
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

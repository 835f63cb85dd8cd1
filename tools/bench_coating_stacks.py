#!/usr/bin/env python3
"""Cost of multilayer coatings (csrc/coating_stack.hpp) next to the single film, one JSON line, also written to
profiles/bench_coating_stacks.json.

    python tools/bench_coating_stacks.py [--reps 5] [--width 1920 --height 1080 --spp 2] [--pairs 4] [--points 32768 --aims 16]

Per camera (C3 DOUBLE_GAUSS and C2 TESSAR, STRICT, every glass given V = 50 where the prescription has none) each of the four passes
that price an interface, once with a 1.38 quarter-wave film at 550 nm on every glass-air interface (the plain kernels) and once with the three-layer
quarter / half / quarter stack (1.38, 2.05, 1.63 at 550 nm, the low index towards the air) on the same interfaces (the stack-aware
kernels); cemented interfaces stay bare in both:
  transmittance   zoic_ray_transmittance_device on the spectral forward records of a frame of synthetic samples, wavelengths uniform
                  in [400, 700] nm
  ghosts          zoic_create_ghost_rays_device, --pairs pairs of zoic_camera_get_ghost_pairs, on a sixteenth of those records
  trace-back      zoic_trace_back_transmittance_spectral_device on the records
  splats          zoic_splat_transmittance_spectral_device, --points scene points as tools/bench_splats.py places them, --aims aims
Every call is timed with device events after one warm-up, mean over --reps calls, in one run on one stream.  ratio: the stack's time over
the film's.  No ratio is asserted.  median_T and the ghosts' median weight are reported for both coatings: the stack has to move them.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "bench_coating_stacks.json")
QHQ = [(1.38, 550.0 / (4 * 1.38)), (2.05, 550.0 / (2 * 2.05)), (1.63, 550.0 / (4 * 1.63))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--aims", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_coating_stacks: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n, k, m = a.width * a.height * a.spp, a.points, a.aims
    ng = n // 16
    smp = torch.empty((n, 4), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(1)
    lam = torch.from_numpy(rng.uniform(400.0, 700.0, n).astype(np.float32)).to(dev)
    plam = torch.from_numpy(rng.uniform(400.0, 700.0, k).astype(np.float32)).to(dev)

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

    result = {"tool": "bench_coating_stacks", "frame": [a.width, a.height, a.spp], "rays": n, "ghost_rays": ng, "pairs": a.pairs, "points": k,
              "aims": m, "cameras": []}
    for name in ("C3", "C2"):
        p = camera_params(name)
        cam = ZoicCamera(device=0)
        if p.get("useImage"):
            cam.set_bokeh_image(hexagon_bokeh())
        cam.set_precision(PRECISION_STRICT)
        cam.update(**p)
        disp = cam.dispersion()
        if not disp["cauchy_b"].any():
            cam.set_abbe_numbers(np.full(len(disp["ior_d"]), 50.0, np.float32))
        st = cam._lib.zoic_generate_samples_device(cam._h, n, 0, a.width, a.height, a.spp, 1, smp.data_ptr(), None)
        assert st == 0, st
        rays = cam.create_rays(smp, wavelengths=lam)["rays"]
        every = cam.ghost_pairs()
        pairs = every[np.linspace(0, len(every) - 1, a.pairs).astype(int)]
        field = 0.5 * float(p["sensorWidth"]) / float(p["focalLength"])
        depth = 10.0 ** rng.uniform(np.log10(20.0), 3.0, k)
        pts_h = np.stack([rng.uniform(-0.8, 0.8, k) * field * depth, rng.uniform(-0.5, 0.5, k) * field * depth, -depth], 1).astype(np.float32)
        pts = torch.from_numpy(pts_h).to(dev)
        u = torch.from_numpy(rng.random((k, m, 2), dtype=np.float32)).to(dev)
        with torch.cuda.stream(stream):
            bounds = cam.pupil_bounds(pts, 16, None, plam)
        stream.synchronize()
        rear = disp["ior_d"].astype(np.float64)                       # trace order; the setters take file order
        front = np.append(rear[1:], 1.0)
        glass_air = (rear != front) & ((rear == 1.0) | (front == 1.0))
        film = np.where(glass_air, np.float32(1.38), np.float32(0.0))[::-1]
        stacks = [(QHQ if f < r else QHQ[::-1]) if ga else None for r, f, ga in zip(rear, front, glass_air)][::-1]
        T = torch.empty((n,), dtype=torch.float32, device=dev)
        G = torch.empty((ng, len(pairs), 8), dtype=torch.float32, device=dev)
        Tb, scr, fl = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev), \
            torch.empty((n,), dtype=torch.int32, device=dev)
        Ts = torch.empty((k, m), dtype=torch.float32, device=dev)
        s = stream.cuda_stream
        runs = {}
        for coating in ("film", "stack"):
            cam.set_coatings(film, 550.0)
            cam.set_coating_stacks(stacks if coating == "stack" else None)
            t = {"transmittance_ms": timed(lambda: cam.transmittance(smp, rays, wavelengths=lam, out=T, stream=s)),
                 "ghosts_ms": timed(lambda: cam.create_ghost_rays(smp[:ng], rays[:ng], pairs, wavelengths=lam[:ng], out=G, stream=s)),
                 "trace_back_ms": timed(lambda: cam.trace_back_transmittance(rays, lam, out=Tb, screen=scr, flags=fl, stream=s)),
                 "splats_ms": timed(lambda: cam.splat_transmittance(pts, bounds, u, plam, out=Ts, stream=s))}
            traced = G[:, :, 7].view(torch.int32) == 1
            t = {key: round(v, 4) for key, v in t.items()}
            t.update(median_T=round(float(T[T > 0].median().item()), 4), median_T_back=round(float(Tb[Tb > 0].median().item()), 4),
                     median_ghost_weight=float("%.3e" % G[:, :, 6][traced].median().item()), ghosts_traced=round(float(traced.float().mean().item()), 4))
            runs[coating] = t
        ratio = {key[:-3]: round(runs["stack"][key] / runs["film"][key], 3) for key in runs["film"] if key.endswith("_ms")}
        result["cameras"].append({"camera": name, "lens": os.path.basename(p["lensDataPath"]), "coated_interfaces": int(glass_air.sum()), "film": runs["film"], "stack": runs["stack"],
                                  "ratio": ratio})
        cam.close()
    line = json.dumps(result)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

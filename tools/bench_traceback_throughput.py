#!/usr/bin/env python3
"""Cost of the trace-back transmittance next to the backward calls it rides on, one JSON line.

    python tools/bench_traceback_throughput.py [--reps 5] [--width 1920 --height 1080 --spp 2] [--points 32768 --aims 16]

Per camera (C3 DOUBLE_GAUSS and C2 TESSAR, STRICT, every glass given V = 50 where the prescription has none), bare and with a 1.38 film
at 550 nm on every interface between unequal media:
  ray side    zoic_trace_back_transmittance_spectral_device against zoic_trace_back_rays_spectral_device on the same rays: the spectral
              forward records of a frame of synthetic samples at wavelengths uniform in [400, 700] nm (48 bytes moved per ray by the
              yardstick, 52 by the new call: one float more).
  splat side  zoic_splat_transmittance_spectral_device against zoic_splat_points_spectral_device on the same points and u: --points
              scene points as tools/bench_splats.py places them, bounded once at lattice 16, --aims aims each (the yardstick writes
              32 bytes per splat, the new call 4).
Every call is timed with device events after one warm-up, mean over --reps calls, in one run on one stream.  ratio: the new call's
time over the yardstick's.  The tool checks that each pair agrees: screen samples and flags bit for bit on the ray side, T > 0 exactly
where the splat record is traced on the splat side.  A single run; the buffers are re-read on every repetition.
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--aims", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_traceback_throughput: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n, k, m = a.width * a.height * a.spp, a.points, a.aims
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

    result = {"tool": "bench_traceback_throughput", "frame": [a.width, a.height, a.spp], "rays": n, "points": k, "aims": m, "cameras": []}
    for name, cfg in (("C3", "C3"), ("C2", "C2")):
        p = camera_params(cfg)
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
        field = 0.5 * float(p["sensorWidth"]) / float(p["focalLength"])
        depth = 10.0 ** rng.uniform(np.log10(20.0), 3.0, k)
        pts_h = np.stack([rng.uniform(-0.8, 0.8, k) * field * depth, rng.uniform(-0.5, 0.5, k) * field * depth, -depth], 1).astype(np.float32)
        pts = torch.from_numpy(pts_h).to(dev)
        u = torch.from_numpy(rng.random((k, m, 2), dtype=np.float32)).to(dev)
        with torch.cuda.stream(stream):
            bounds = cam.pupil_bounds(pts, 16, None, plam)
        stream.synchronize()
        ior = disp["ior_d"]                       # trace order; set_coatings takes file order
        differ = ior != np.append(ior[1:], np.float32(1.0))
        film = np.where(differ, np.float32(1.38), np.float32(0.0))[::-1]
        row = {"camera": name, "lens": os.path.basename(p["lensDataPath"]), "runs": []}
        for coated in (False, True):
            cam.set_coatings(film if coated else None, 550.0 if coated else None)
            scr, fl = torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            T, scr2, fl2 = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty_like(scr), torch.empty_like(fl)
            tb = timed(lambda: cam.trace_back(rays, out=scr, flags=fl, stream=stream.cuda_stream, wavelengths=lam))
            tt = timed(lambda: cam.trace_back_transmittance(rays, lam, out=T, screen=scr2, flags=fl2, stream=stream.cuda_stream))
            same = bool(torch.equal(fl, fl2)) and bool(torch.equal(scr.view(torch.int32), scr2.view(torch.int32)))
            same = same and bool(torch.equal(T > 0, (fl & 1) == 1))
            assert same, (name, coated)
            traced = (fl & 1) == 1
            rec = torch.empty((k, m, 8), dtype=torch.float32, device=dev)
            Ts = torch.empty((k, m), dtype=torch.float32, device=dev)
            sp = timed(lambda: cam.splat_points(pts, bounds, u, plam, out=rec, stream=stream.cuda_stream))
            st_ms = timed(lambda: cam.splat_transmittance(pts, bounds, u, plam, out=Ts, stream=stream.cuda_stream))
            same_splat = bool(torch.equal(Ts > 0, (rec[:, :, 6].view(torch.int32) & 1) == 1))
            assert same_splat, (name, coated)
            row["runs"].append({
                "film": coated,
                "rays": {"n": n, "traced": round(float(traced.float().mean().item()), 5), "median_T": round(float(T[traced].median().item()), 4),
                         "trace_back_spectral_ms": round(tb, 4), "transmittance_ms": round(tt, 4),
                         "Grays_per_s": round(n / tt / 1e6, 3), "ratio": round(tt / tb, 3), "same_Ps_flags": same},
                "splats": {"n": k * m, "traced": round(float((Ts > 0).float().mean().item()), 5),
                           "splat_points_spectral_ms": round(sp, 4), "transmittance_ms": round(st_ms, 4),
                           "Gsplats_per_s": round(k * m / st_ms / 1e6, 3), "ratio": round(st_ms / sp, 3), "same_traced": same_splat}})
        result["cameras"].append(row)
        cam.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

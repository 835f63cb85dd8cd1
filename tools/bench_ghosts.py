#!/usr/bin/env python3
"""Cost of the ghost pass (zoic_create_ghost_rays_device) at p = 1, 8 and all reflecting pairs of the lens, bare and coated, beside
the Fresnel transmittance pass (zoic_ray_transmittance_device, k = 1) over the same samples' records, taken in the same run: C2 and
C3 (V = 50 for every glass), one JSON line, also written to profiles/bench_ghosts.json.

    python tools/bench_ghosts.py [--reps 3] [--precision fast|strict] [--max-rays N] [--out profiles/bench_ghosts.json]

Per config the frame's first --max-rays samples are synthesised on the device; the wavelengths are uniform in [400, 700] nm.  The
spectral call writes the n records, then the passes over them are timed with device events on one stream, after one warm-up:
    ghost  p = 1 (the first pair of ghost_pairs()), p = 8 (its first eight) and all pairs (in calls of at most 32), each bare and with
           a 1.38-index film, a quarter wave thick at 550 nm, on every interface
    trans  the transmittance pass, bare and with the same film
Each is the mean over --reps runs.  ns_per_visit divides by the interface visits of the paths that came THROUGH: for a traced ghost of
the pair (a, b) on a lens of `count` interfaces (a + 1) + (a - b) + (count - 1 - b), for a transmittance column with T > 0 `count`.  The
visits a ghost makes before it is clipped are work too but are not counted, so the ghost pass's figure is an upper bound of its cost
per visit; traced_frac says how many ghosts came through.  The ghost pass also writes 32 bytes per (sample, pair), the transmittance
pass 4 per sample.  No ratio is asserted anywhere.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ABBE = {"C3": 50.0}   # the double Gauss ships no V-numbers


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ghosts.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zoic_amd import PRECISION_FAST, PRECISION_STRICT, ZoicCamera
    from zoic_amd.workloads import CONFIGS, camera_params, hexagon_bokeh
    if not torch.cuda.is_available():
        sys.exit("bench_ghosts: no GPU visible (nothing measured)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    result = {"tool": "bench_ghosts", "precision": a.precision, "wavelengths_nm": [400, 700], "film": [1.38, 550.0], "reps": a.reps, "configs": []}
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
        every = cam.ghost_pairs()
        g = torch.Generator(device=dev)
        g.manual_seed(4)
        st = stream.cuda_stream
        row = {"config": cfg, "samples": n, "interfaces": int(count), "pairs": int(len(every)), "ghost": {}}
        with torch.cuda.stream(stream):
            s = cam.generate_samples(n, c["width"], c["height"], c["spp"], seed=1, stream=st)
            lam = torch.empty((n,), dtype=torch.float32, device=dev).uniform_(400.0, 700.0, generator=g)
            rays = cam.create_rays(s, wavelengths=lam, stream=st)["rays"]
            live = int((rays[:, 6] != 0).sum())
            row["live_frac"] = round(live / n, 4)
            t_out = torch.empty((n,), dtype=torch.float32, device=dev)
            run_t = lambda: cam.transmittance(s, rays, wavelengths=lam, out=t_out, stream=st)   # noqa: E731
            trans = {}
            for name, coat in (("bare", None), ("film", film)):
                cam.set_coatings(coat, None if coat is None else 550.0)
                ms = timed(torch, stream, a.reps, run_t)
                visits = int((t_out > 0).sum()) * int(count)
                trans[name] = {"ms": round(ms, 3), "visits": visits, "ns_per_visit": round(ms * 1e6 / max(visits, 1), 4)}
            row["trans"] = trans
            for label, pairs in (("1", every[:1]), ("8", every[:8]), ("all", every)):
                chunks = [pairs[lo:lo + 32] for lo in range(0, len(pairs), 32)]
                outs = [torch.empty((n, len(q), 8), dtype=torch.float32, device=dev) for q in chunks]

                def run_g():
                    for q, o in zip(chunks, outs):
                        cam.create_ghost_rays(s, rays, q, wavelengths=lam, out=o, stream=st)

                per_pair = np.array([(pa + 1) + (pa - pb) + (count - 1 - pb) for pa, pb in pairs], np.int64)
                r = {"p": int(len(pairs))}
                for name, coat in (("bare", None), ("film", film)):
                    cam.set_coatings(coat, None if coat is None else 550.0)
                    ms = timed(torch, stream, a.reps, run_g)
                    traced = torch.cat([(o[:, :, 7].view(torch.int32) & 1).sum(0) for o in outs]).cpu().numpy().astype(np.int64)
                    visits = int((traced * per_pair).sum())
                    r[name] = {"ms": round(ms, 3), "ns_per_ghost": round(ms * 1e6 / (n * len(pairs)), 4), "traced_frac": round(float(traced.sum()) / (n * len(pairs)), 4),
                               "visits": visits, "ns_per_visit": round(ms * 1e6 / max(visits, 1), 4)}
                row["ghost"][label] = r
                del outs
                torch.cuda.empty_cache()
            cam.set_coatings(None, None)
        result["configs"].append(row)
        cam.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

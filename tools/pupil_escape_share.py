"""How much of the pupil the grown `aim` box of the pupil bounds misses, on the CPU: for the test cameras and points
(tests/pupil_cases.py) and each lattice size, random aims uniform on the front square are traced back from the point by the host
build of csrc/traceback.hpp; of those that are traced back, the share that lies outside the point's grown box is the escape share.
Also printed: the share of traced aims among draws in the box against draws in the whole square (what the box buys).

    python tools/pupil_escape_share.py [--aims 20000]      (per point; 8 points per camera)

Needs no GPU: a tables-only camera and the tests' host drivers."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import host_drivers  # noqa: E402
import pupil_cases as pc  # noqa: E402
import pupil_driver  # noqa: E402
import pupil_ref  # noqa: E402
import traceback_cases as tc  # noqa: E402
from zoic_amd import ZoicCamera, pupil_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aims", type=int, default=20000, help="random aims per point")
    a = ap.parse_args()
    drv, tdrv = pupil_driver.pupil(), host_drivers.traceback()
    rng = np.random.default_rng(2)
    print("%-14s %3s %9s %9s %10s %10s %10s" % ("camera", "G", "aims", "traced", "escaped", "in square", "in box"))
    for name in pc.CAMERAS:
        p = pc.params_of(name)
        cam = tc.update(ZoicCamera(device=-1), p)
        z, R = pupil_ref.square(cam.info(), p)
        pts = pc.points(p)[:pc.BEHIND]
        u = rng.random((len(pts), a.aims, 2))
        o = np.repeat(pts, a.aims, axis=0)
        A = np.concatenate([(2.0 * u.reshape(-1, 2) - 1.0) * float(R), np.full((len(o), 1), float(z))], 1).astype(np.float32)
        _, fl = host_drivers.drive_traceback(tdrv, cam, p, o, o - A)
        traced = ((fl & 1) == 1).reshape(len(pts), a.aims)
        Axy = A[:, :2].reshape(len(pts), a.aims, 2)
        for G in pc.LATTICES:
            b = pupil_driver.drive_pupil(drv, cam, p, pts, G)
            lo, hi = b["aim"][:, None, 0:2], b["aim"][:, None, 2:4]
            inside = ((Axy >= lo) & (Axy <= hi)).all(2) & (b["count"] > 0)[:, None]
            escaped = traced & ~inside
            _, d, _ = pupil_rays(o, np.repeat(b, a.aims), u.reshape(-1, 2), float(z))
            _, fb = host_drivers.drive_traceback(tdrv, cam, p, o, d)
            box = ((fb & 1) == 1).reshape(len(pts), a.aims)[b["count"] > 0]
            print("%-14s %3d %9d %9d %9.4f%% %9.4f%% %9.4f%%" % (name, G, traced.size, traced.sum(), 100.0 * escaped.sum() / max(1, traced.sum()),
                                                              100.0 * traced.mean(), 100.0 * box.mean() if box.size else 0.0))
        cam.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the finite projection: the potential build per frame with and without msl_set_projection, on one
handle per state, interleaved.  bench.py is not touched.

    python tools/finite_projection_bench.py                       # 512^2 x 100 and 1024^2 x 200, (R, J) = (2, 2) and (4, 4)
    python tools/finite_projection_bench.py --shapes 512x100 --settings 2x2 --reps 5 --out profiles/finite_projection.txt

Atoms: uniformly random at hBN's density (two species), 0.1 A pixels, 0.5 A slices.  Prints and writes one line per shape and setting:
ms per build (device time, the library's HIP-event counters: median and spread over the repeats), the ratio to the build without
the option and the expected 2 (2 R + 1).  --off-only times the build without the option alone, with a binding that may predate the
option (the same measurement on the parent commit)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x100,1024x200", help="comma-separated NxSLICES")
    ap.add_argument("--settings", default="2x2,4x4", help="comma-separated RxJ")
    ap.add_argument("--density", type=float, default=0.1, help="atoms per cubic Angstrom")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "finite_projection.txt"))
    a = ap.parse_args()
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import loadKirkland, slice_edges
    d, dz, eV = 0.1, 0.5, 100e3
    lines = []
    for shape in a.shapes.split(","):
        n, nz = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(0)
        n_atoms = int(round(a.density * (n * d) ** 2 * nz * dz))
        pos = rng.random((n_atoms, 3)) * np.array([n * d, n * d, nz * dz])
        Z = np.array([5, 7], dtype=np.int32)[np.arange(n_atoms) % 2]
        settings = [(0, 1)] + ([] if a.off_only else [tuple(int(v) for v in s.split("x")) for s in a.settings.split(",")])
        engines = {}
        for R, J in settings:
            eng = _native.Engine(n, n, nz, d, d, dz, wavelength(eV), interaction_sigma(eV), launch_timing=True)
            eng.set_kirkland(loadKirkland())
            eng.set_slices(*slice_edges(np.arange(nz) * dz))
            if R:
                eng.set_projection(R, J)
            engines[R, J] = eng
        ms = {k: [] for k in engines}
        for rep in range(a.warmup + a.reps):                    # interleaved: off, (2, 2), (4, 4), off, ...
            for key, eng in engines.items():
                eng.reset_counters()
                eng.build_potential(pos, Z)
                eng.synchronize()
                if rep >= a.warmup:
                    ms[key].append(eng.counters()["ms_potential"])
        for eng in engines.values():
            eng.close()
        off = float(np.median(ms[0, 1]))
        for (R, J), v in ms.items():
            med, spread = float(np.median(v)), float(np.max(v) - np.min(v))
            what = "infinite projection (option off)" if R == 0 else f"finite projection R={R} J={J}"
            tail = "" if R == 0 else f"  ratio {med / off:6.2f}  (expected about 2 (2 R + 1) = {2 * (2 * R + 1)})"
            lines.append(f"{n}^2 x {nz} slices, {n_atoms} atoms: {what}: build {med:9.3f} ms per frame (spread {spread:.3f} over {a.reps}){tail}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

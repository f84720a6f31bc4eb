#!/usr/bin/env python3
"""Cost of the band limit: the potential build per frame and the slice loop per slice-step, with and without
msl_set_bandlimit, on one handle per state, interleaved.  The shape comes from the arguments; bench.py is not touched.

    python tools/bandlimit_bench.py --n 1024 --slices 50 --probes 64 --atoms 20000 --reps 5
    python tools/bandlimit_bench.py --n 512 --slices 100 --probes 1 --atoms 50000

Prints one JSON line: ms per build and per slice loop (device time, the library's HIP-event counters), the ratios, the cuts."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fraction", type=float, default=2.0 / 3.0)
    ap.add_argument("--sampling", type=float, default=0.1)
    a = ap.parse_args()
    from pyslice_amd import _native
    from pyslice_amd.bandlimit import BandLimit
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import loadKirkland, slice_edges
    nx, ny, nz, d, dz, eV = a.n, a.ny or a.n, a.slices, a.sampling, 2.0, 100e3
    rng = np.random.default_rng(0)
    pos = rng.random((a.atoms, 3)) * np.array([nx * d, ny * d, nz * dz])
    Z = rng.choice(np.array([6, 14, 29], dtype=np.int32), a.atoms)
    xy = rng.random((a.probes, 2)) * np.array([nx * d, ny * d])
    cuts = BandLimit(a.fraction).cuts(nx, ny, d, d)
    engines = {}
    for name in ("off", "on"):
        eng = _native.Engine(nx, ny, nz, d, d, dz, wavelength(eV), interaction_sigma(eV), n_probes=a.probes, launch_timing=True)
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(np.arange(nz) * dz))
        if name == "on":
            eng.set_bandlimit(*cuts)
        eng.set_probes(20.0, xy)
        engines[name] = eng
    ms = {k: {"build": [], "loop": []} for k in engines}
    for rep in range(a.warmup + a.reps):                    # interleaved: off, on, off, on, ...
        for name, eng in engines.items():
            eng.reset_counters()
            eng.build_potential(pos, Z)
            eng.propagate()
            eng.synchronize()
            c = eng.counters()
            if rep >= a.warmup:
                ms[name]["build"].append(c["ms_potential"])
                ms[name]["loop"].append(c["ms_propagate"])
    for eng in engines.values():
        eng.close()
    med = {k: {w: float(np.median(v)) for w, v in m.items()} for k, m in ms.items()}
    spread = {k: {w: float(np.max(v) - np.min(v)) for w, v in m.items()} for k, m in ms.items()}
    print(json.dumps({"nx": nx, "ny": ny, "slices": nz, "probes": a.probes, "atoms": a.atoms, "cuts": cuts, "reps": a.reps,
                      "build_ms": {k: med[k]["build"] for k in med}, "build_ratio": med["on"]["build"] / med["off"]["build"],
                      "loop_ms": {k: med[k]["loop"] for k in med}, "loop_ratio": med["on"]["loop"] / med["off"]["loop"],
                      "loop_us_per_slice_step": {k: 1e3 * med[k]["loop"] / (nz * a.probes) for k in med},
                      "spread_ms": spread}))


if __name__ == "__main__":
    main()

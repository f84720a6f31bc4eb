"""Time the potential build of frozen-phonon configurations: msl_build_thermal (positions generated on the device from the resident
structure) against msl_build_potentials fed the same configurations from a (B, n_atoms, 3) host array.

    python tools/thermal_bench.py [--reps 20] [--out profiles/thermal_build.txt]
    MSL_LIB=/path/to/parent/libmslice.so python tools/thermal_bench.py --parent        # the same host-fed build on an older library

Each timing is ONE synchronous call per frame batch: the call plus msl_synchronize, wall clock, so that the host's share (the
pageable -> pinned memcpy and the H2D copy of stage_atoms against nothing) is in it.  Two shapes: C2 (512^2 x 100 slices) and a
many-atom case (1024^2 x 200 slices), both at the benchmark's atom density.  Prints the median, minimum and maximum of the
repetitions; the ratio printed is median build_thermal / median build_potentials of the same library; the one against the parent's
library is taken from the two runs' lines."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THERMAL = ("msl_set_structure", "msl_build_thermal", "msl_thermal_positions")
CASES = [("C2", 512, 100, 32), ("many-atom", 1024, 200, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.08)
    ap.add_argument("--parent", action="store_true", help="the library (MSL_LIB) predates the thermal entry points: time build_potentials only")
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    import numpy as np
    from pyslice_amd import _native, thermal
    if a.parent:
        # the parent's library lacks the three entry points the binding asks every library for: give load() stand-ins for them
        # (never called here), so that the binding itself stays strict
        import ctypes

        class ParentLibrary(ctypes.CDLL):
            def __getattr__(self, name):
                if name in THERMAL:
                    return type("absent", (), {})()
                return super().__getattr__(name)
        ctypes.CDLL = ParentLibrary
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import gridFromTrajectory, loadKirkland, slice_edges
    from pyslice_amd.synthetic import synthetic_trajectory
    lines = [f"# library {_native.LIB_PATH}{' (parent: host-fed build only)' if a.parent else ''}; {a.reps} synchronous calls per line after "
             f"{a.warmup} warm-up calls; ms per call of one frame batch"]

    def timed(call, eng):
        for _ in range(a.warmup):
            call()
            eng.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            eng.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    for name, n, nz, B in CASES:
        tr = synthetic_trajectory(n, nz, 1, seed=3)
        xs, ys, zs = gridFromTrajectory(tr)[:3]
        Z = np.asarray(tr.atom_types, dtype=np.int32)
        sigma = np.full(len(Z), a.sigma)
        host = np.stack([thermal.displaced(tr.positions[0], sigma, 11, 100 + k) for k in range(B)])
        eng = _native.Engine(n, n, nz, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(100e3), interaction_sigma(100e3), n_probes=1,
                             n_frames=1, frame_batch=B)
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(zs))
        head = f"{name}: {n}^2 x {nz} slices, {len(Z)} atoms, frame batch {B} ({host.nbytes / 1e6:.1f} MB of positions per call)"
        med_p, lo, hi = timed(lambda: eng.build_potentials(host, Z), eng)
        lines.append(f"{head}: build_potentials median {med_p:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        if not a.parent:
            eng.set_structure(tr.positions[0], Z, sigma)
            med_t, lo, hi = timed(lambda: eng.build_thermal(11, 100, B), eng)
            lines.append(f"{head}: build_thermal    median {med_t:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
                         f"build_thermal / build_potentials of this library = {med_t / med_p:.3f}")
        eng.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

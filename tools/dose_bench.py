"""Finite dose on the device, measured: msl_dose_counts alone at a few levels of lam (inversion and PTRS cost differently), and
run_diffraction() with and without a dose on one scan, with the bytes each downloads per probe.

    python tools/dose_bench.py [--grid 256] [--window 128] [--slices 20] [--scan 16] [--frames 4] [--frame-batch N] [--out profiles/dose_counts.txt]

Times are host clocks around calls that end in a stream synchronise (msl_dose_counts downloads its counts); every shape is run once
before it is timed.  Needs an MI355X: there is no CPU path."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_counts(lines, B, wx, wy, reps):
    """msl_dose_counts of a (B, wx, wy) accumulator filled with |Psi|^2 = 1 per pixel of one frame, at scale = lam"""
    import torch
    from pyslice_amd import _native
    eng = _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        d = torch.ones((B, 1, wx * wy), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        eng.dose_reset(B, (wx, wy))
        eng.dose_add(0, 1, src=(d.data_ptr(), B, 1, wx, wy))
        n = B * wx * wy
        lines.append(f"msl_dose_counts alone: {B} probes x {wx} x {wy} = {n} pixels, counts downloaded ({4 * n / 1e6:.1f} MB), "
                     f"median of {reps} calls")
        for lam in (0.01, 1.0, 9.0, 10.0, 100.0, 1e4, 1e6):
            eng.dose_counts(lam, 1, B=B)
            ts = []
            for r in range(reps):
                t0 = time.perf_counter()
                counts, _ = eng.dose_counts(lam, 2 + r, B=B)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            lines.append(f"  lam {lam:>9g} ({'PTRS' if lam >= 10 else 'inversion'}): {t * 1e3:8.3f} ms  {n / t / 1e9:6.2f} Gpixel/s  "
                         f"mean count {counts.mean():.4g}")
        eng.dose_counts(1.0, 1, B=B, keep_intensity=True)
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            eng.dose_counts(1.0, 2 + r, B=B, keep_intensity=True)
            ts.append(time.perf_counter() - t0)
        lines.append(f"  lam 1 with the float64 sums downloaded as well ({12 * n / 1e6:.1f} MB): {float(np.median(ts)) * 1e3:8.3f} ms")
    finally:
        eng.close()


def time_scan(lines, a):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(a.grid, a.slices, a.frames, density=0.1, seed=3)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    g = (np.arange(a.scan) + 0.5) / a.scan
    pp = [(x * lx, y * ly) for x in g for y in g]
    win = (a.window, a.window)
    mx = a.window
    lines.append(f"run_diffraction(): grid {a.grid}^2, {a.slices} slices, {a.frames} frames, {len(pp)} probes, k_window {win}, bin (1, 1), "
                 f"probe_batch {a.probe_batch}, best of {a.reps}")
    cases = (("no dose", None), ("dose, counts only", ps.Dose(electrons_per_probe=1e5, seed=1)),
             ("dose, keep_intensity", ps.Dose(electrons_per_probe=1e5, seed=1, keep_intensity=True)))
    for name, dose in cases:
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(dose=dose), k_window=win, probe_batch=a.probe_batch,
                                       frame_batch=a.frame_batch)
        calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        calc.run_diffraction()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dd = calc.run_diffraction()
            ts.append(time.perf_counter() - t0)
        # without a dose every frame batch downloads the float64 patterns of the probe batch; with one, one download per probe
        n_fb = len(calc._frame_batches())
        per_probe = 8 * mx * mx * n_fb if dose is None else (4 + (8 if dose.keep_intensity else 0)) * mx * mx
        builds = n_fb if dose is None or a.frames <= calc._engine.frame_batch else n_fb * -(-len(pp) // calc.probe_batch)
        lines.append(f"  {name:22s}: {min(ts):7.3f} s  ({min(ts) / len(pp) * 1e3:6.2f} ms per probe)  {per_probe / 1e3:8.1f} kB downloaded "
                     f"per probe, result {per_probe // n_fb if dose is None else per_probe} B per probe on the host, "
                     f"{builds} potential builds (frame batch {calc._engine.frame_batch})")
        if dose is not None:
            lines.append(f"  {'':22s}  electrons counted per probe: mean {dd.counts.sum(axis=(-2, -1)).mean():.1f} of {dd.electrons_per_probe:g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--slices", type=int, default=20)
    ap.add_argument("--scan", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--probe-batch", type=int, default=64)
    ap.add_argument("--frame-batch", type=int, default=None, help="default: chosen by setup()")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    time_counts(lines, 64, 128, 128, 7)
    time_scan(lines, a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Detector response on the device, measured: msl_dose_frames against msl_dose_counts on the same accumulator, the camera pass
against a device copy of the same bytes, and run_diffraction() with a camera against the same scan with the dose alone.

    python tools/camera_bench.py [--out profiles/camera_frames.txt]              the calls, then the scan in this process
    python tools/camera_bench.py --calls-only [--pixels 4]                       the calls alone (for a kernel trace)
    python tools/camera_bench.py --against DIR [--rounds 4]                      the scan, alternating with the checkout in DIR

--against DIR starts one fresh process per run: the dose-alone scan on the package in DIR (a checkout of the parent commit, built),
then the camera scan and the dose-alone scan on this tree, --rounds times over; the spread of DIR's own runs is the yardstick.
Times are host clocks around calls that end in a stream synchronise (both calls download their result); every shape is run once
before it is timed.  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_calls(lines, mpix, reps, radii=(0, 2, 4, 8)):
    """msl_dose_counts and msl_dose_frames (each with its download) on one accumulator of mpix million pixels of lam = 20"""
    import torch
    from pyslice_amd import _native
    from pyslice_amd.camera import Camera, gaussian_psf
    wx = wy = 256
    B = max(1, round(mpix * 1e6 / (wx * wy)))
    n = B * wx * wy
    eng = _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        d = torch.ones((B, 1, wx * wy), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        eng.dose_reset(B, (wx, wy))
        eng.dose_add(0, 1, src=(d.data_ptr(), B, 1, wx, wy))
        del d

        def median(call):
            call(1)
            ts = []
            for r in range(reps):
                t0 = time.perf_counter()
                call(2 + r)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts))
        t_counts = median(lambda seed: eng.dose_counts(20.0, seed, B=B))
        lines.append(f"{B} patterns of {wx} x {wy} = {n / 1e6:.2f} Mpixel, lam 20, median of {reps} calls")
        lines.append(f"  msl_dose_counts (4 B/pixel down)      : {t_counts * 1e3:8.3f} ms  {t_counts * 1e9 / n:7.4f} ms per Mpixel")
        for r in radii:
            eng.set_camera(Camera(gaussian_psf(max(r, 1) / 3.0, r), gain=2.5, offset=20.0, readout_noise=1.5))
            t = median(lambda seed: eng.dose_frames(20.0, seed, B=B))
            lines.append(f"  msl_dose_frames r = {r} (2 B/pixel down) : {t * 1e3:8.3f} ms  {t * 1e9 / n:7.4f} ms per Mpixel  "
                         f"{t / t_counts:5.2f} x msl_dose_counts")
        # a device copy that moves the bytes of the camera pass: 4 B read and 2 B written per pixel = 3 B copied per pixel
        src = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for r in range(reps):
            dst.copy_(src)
            ev[r + 1].record()
        torch.cuda.synchronize()
        t_copy = float(np.median([ev[r].elapsed_time(ev[r + 1]) for r in range(reps)]))
        lines.append(f"  device copy of {3 * n / 1e6:.1f} MB (6 B/pixel moved) : {t_copy:8.4f} ms  {6 * n / t_copy / 1e9:7.1f} TB/s  (device events)")
    finally:
        eng.close()


def scan_setup(a, camera):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(a.grid, a.slices, a.frames, density=0.1, seed=3)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    g = (np.arange(a.scan) + 0.5) / a.scan
    pp = [(x * lx, y * ly) for x in g for y in g]
    dose = ps.Dose(electrons_per_probe=1e5, seed=1)
    if camera:
        diffraction = ps.Diffraction(dose=dose, camera=ps.Camera(ps.gaussian_psf(1.0), gain=2.5, offset=20.0, readout_noise=1.5))
    else:
        diffraction = ps.Diffraction(dose=dose)
    calc = ps.MultisliceCalculator(progress=False, diffraction=diffraction, k_window=(a.window, a.window), probe_batch=a.probe_batch,
                                   frame_batch=a.frame_batch)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    return calc


def time_scan(a, camera):
    """seconds of a.reps calls of run_diffraction() after one warm-up call"""
    calc = scan_setup(a, camera)
    calc.run_diffraction()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dd = calc.run_diffraction()
        ts.append(time.perf_counter() - t0)
    arr = dd.frames if camera else dd.counts
    return ts, int(arr.nbytes // arr.shape[0])


def scan_text(a):
    return (f"grid {a.grid}^2, {a.slices} slices, {a.frames} frames, {a.scan} x {a.scan} probes, k_window ({a.window}, {a.window}), "
            f"probe_batch {a.probe_batch}, frame_batch {a.frame_batch}")


def against(lines, a):
    args = [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("grid", "window", "slices", "scan", "frames", "probe_batch", "frame_batch", "reps")]
    me = os.path.abspath(__file__)
    runs = {"parent, dose alone": [], "this tree, dose alone": [], "this tree, camera": []}

    def one(name, tree, camera):
        cmd = [sys.executable, me, "--one-scan", "--tree", tree] + (["--camera"] if camera else []) + args
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
        runs[name].append(json.loads(out.strip().splitlines()[-1])["seconds"])
    for _ in range(a.rounds):
        one("parent, dose alone", os.path.abspath(a.against), False)
        one("this tree, camera", HERE, True)
        one("this tree, dose alone", HERE, False)
    lines.append(f"run_diffraction(): {scan_text(a)}; {a.rounds} fresh processes each, alternating, {a.reps} timed calls per process")
    best = {}
    for name, rs in runs.items():
        per = [min(r) for r in rs]                                  # the best call of every process
        best[name] = float(np.median(per))
        lines.append(f"  {name:22s}: best call per process " + " ".join(f"{t:.4f}" for t in per) + f" s   median {best[name]:.4f} s   "
                     f"spread (max - min) {max(per) - min(per):.4f} s")
    p = best["parent, dose alone"]
    lines.append(f"  camera / parent dose alone: {best['this tree, camera'] / p:.3f}   this tree's dose alone / parent's: "
                 f"{best['this tree, dose alone'] / p:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--scan", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--probe-batch", type=int, default=256)
    ap.add_argument("--frame-batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--pixels", type=float, nargs="*", default=[1, 4, 16], help="millions of pixels of the timed calls")
    ap.add_argument("--call-reps", type=int, default=20)
    ap.add_argument("--against", default=None, help="a built checkout of another commit to alternate the scan with")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--one-scan", action="store_true", help="(used by --against) time the scan once and print one JSON line")
    ap.add_argument("--camera", action="store_true")
    ap.add_argument("--tree", default=HERE, help="(used by --against) the checkout whose package is imported")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.one_scan:
        ts, per_probe = time_scan(a, a.camera)
        print(json.dumps({"seconds": ts, "bytes_per_probe": per_probe}))
        return
    lines = []
    if a.against:
        against(lines, a)
    else:
        for mpix in a.pixels:
            time_calls(lines, mpix, a.call_reps)
        if not a.calls_only:
            lines.append(f"run_diffraction() in this process: {scan_text(a)}, best of {a.reps}")
            for name, camera in (("dose alone", False), ("camera", True)):
                ts, per_probe = time_scan(a, camera)
                lines.append(f"  {name:12s}: {min(ts):7.4f} s  {per_probe / 1e3:6.1f} kB downloaded per probe")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.against else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

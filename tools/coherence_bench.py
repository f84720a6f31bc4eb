"""Partial coherence on the device, measured: msl_diffract_members over a (B, T, K) array against msl_diffract over the same array
plus the host fold of its output, for G in {3, 9, 27}; the two device passes alone in their accumulating forms (msl_dose_add_members
against msl_dose_add: nothing is downloaded, timed alike, queued and with one synchronise per call); and one small run_diffraction()
with and without a Coherence.

    python tools/coherence_bench.py [--waves 216] [--frames 8] [--window 256] [--grid 128] [--slices 20] [--scan 4] [--out profiles/partial_coherence.txt]

Times are host clocks around calls that end in a stream synchronise; every shape is run once before it is timed.  Needs an MI355X:
there is no CPU path."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def time_fold(lines, B, T, w, bin, reps):
    """the pattern pass over (B, T, w * w) complex64 on the device: folded there, or per wave with the fold on the host"""
    import torch
    from pyslice_amd import _native
    from pyslice_amd.coherence import fold_members
    eng = _native.Engine(w, w, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        d = torch.view_as_complex(torch.randn((B, T, w * w, 2), dtype=torch.float32, device="cuda", generator=g))
        torch.cuda.synchronize()
        src = (d.data_ptr(), B, T, w, w)
        mx = w // bin[0]
        read = 8.0 * B * T * w * w
        lines.append(f"pattern pass over {B} waves x {T} frames x {w} x {w} complex64 ({read / 1e6:.1f} MB read), bin {bin}, median of {reps} calls")
        t_plain = _median(lambda: eng.diffract(0, T, bin=bin, src=src), reps)
        lines.append(f"  msl_diffract, {8 * B * mx * mx / 1e6:7.2f} MB downloaded:                {t_plain * 1e3:8.3f} ms   {read / t_plain / 1e9:7.1f} GB/s")

        def device_only(call, each=False, n=50):
            """mean time of n calls that download nothing: queued with one synchronise at the end, or (each) one after every call"""
            eng.dose_reset(B, (mx, mx))
            call()
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                call()
                if each:
                    eng.synchronize()
            eng.synchronize()
            return (time.perf_counter() - t0) / n
        t_acc = device_only(lambda: eng.dose_add(0, T, bin=bin, src=src))
        t_acc1 = device_only(lambda: eng.dose_add(0, T, bin=bin, src=src), each=True)
        lines.append(f"  msl_dose_add (the same pass, nothing downloaded; mean of 50 calls): queued {t_acc * 1e3:8.3f} ms  {read / t_acc / 1e9:7.1f} GB/s"
                     f"   synchronised each {t_acc1 * 1e3:8.3f} ms")
        for G in (3, 9, 27):
            wts = np.full(G, 1.0 / G) * (1.0 + 0.1 * np.cos(np.arange(G)))
            wts /= wts.sum()
            t_dev = _median(lambda: eng.diffract_members(wts, 0, T, bin=bin, src=src), reps)
            t_host = _median(lambda: fold_members(eng.diffract(0, T, bin=bin, src=src), wts), reps)
            same = np.array_equal(eng.diffract_members(wts, 0, T, bin=bin, src=src), fold_members(eng.diffract(0, T, bin=bin, src=src), wts))
            t_macc = device_only(lambda: eng.dose_add_members(wts, 0, T, bin=bin, src=src))
            t_macc1 = device_only(lambda: eng.dose_add_members(wts, 0, T, bin=bin, src=src), each=True)
            lines.append(f"  G = {G:2d}: msl_diffract_members {t_dev * 1e3:8.3f} ms ({8 * B // G * mx * mx / 1e6:6.2f} MB downloaded)   msl_diffract + host fold "
                         f"{t_host * 1e3:8.3f} ms   bitwise equal: {same}")
            lines.append(f"          msl_dose_add_members (nothing downloaded): queued {t_macc * 1e3:8.3f} ms  {read / t_macc / 1e9:7.1f} GB/s  "
                         f"{100.0 * (t_macc / t_acc - 1.0):+6.1f} % against msl_dose_add   synchronised each {t_macc1 * 1e3:8.3f} ms  "
                         f"{100.0 * (t_macc1 / t_acc1 - 1.0):+6.1f} %")
    finally:
        eng.close()


def time_scan(lines, a):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(a.grid, a.slices, 2, density=0.1, seed=3)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    g = (np.arange(a.scan) + 0.5) / a.scan
    pp = [(x * lx, y * ly) for x in g for y in g]
    lines.append(f"run_diffraction(): grid {a.grid}^2, {a.slices} slices, 2 frames, {len(pp)} positions, bin (2, 2), best of {a.reps}")
    cases = (("coherent", None), ("G = 3 (focal)", ps.Coherence(focal_spread=40.0, focal_points=3)),
             ("G = 9 (source)", ps.Coherence(source_size=0.3, source_points=3)),
             ("G = 27", ps.Coherence(focal_spread=40.0, focal_points=3, source_size=0.3, source_points=3)))
    base = None
    for name, c in cases:
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=(2, 2)), coherence=c,
                                       aberrations=ps.Aberrations(C10=-150.0, Cs=2e6))
        calc.setup(tr, aperture=25.0, voltage_eV=100e3, probe_positions=pp)
        calc.run_diffraction()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            calc.run_diffraction()
            ts.append(time.perf_counter() - t0)
        t = min(ts)
        base = t if base is None else base
        G = 1 if c is None else c.n_members
        lines.append(f"  {name:16s}: {t * 1e3:9.3f} ms  ({t / len(pp) * 1e3:7.3f} ms per position, {t / len(pp) / G * 1e3:7.4f} ms per wave)  "
                     f"{t / base:5.1f} x the coherent run, waves per batch {calc.probe_batch}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=216, help="B of the pattern pass: a multiple of 27")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--slices", type=int, default=20)
    ap.add_argument("--scan", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for bin in ((1, 1), (2, 2)):
        time_fold(lines, a.waves, a.frames, a.window, bin, a.reps)
    time_scan(lines, a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

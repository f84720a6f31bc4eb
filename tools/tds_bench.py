"""Cost of the TDS detector signal: run_detectors() with and without tds=True on the same absorptive scan,
and the reduction kernel alone against a device copy of the buffer it reads.

    python tools/tds_bench.py [--out profiles/tds_detector.txt] [--repeat 3] [--grid 512] [--slices 100] [--scan 16]

The scan: scan x scan probe positions, grid^2 pixels of 0.1 A, `slices` slices of 1 A with 40 atoms of Si and O each, probe_batch=64,
two detectors.  The two runs alternate in one session, the calculators set up once each; the figure is the median of run_detectors().
The reduction: msl_tds_reduce repeats the tile kernel (slice_sums_kernel<TdsSums>) 200 times between two events on the 64 exit waves the last slice loop left
(8 bytes per pixel and image read); the copy is torch's device-to-device copy of a buffer of the same size (8 bytes read and 8
written), timed the same way in the same session."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EV = 100e3


def source(n, nz):
    from pyslice_amd.absorptive import AbsorptivePotential
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(n, nz, 0.1, 1.0, n)
    rng = np.random.default_rng(5)
    pos = rng.random((40 * nz, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, len(pos))]
    return AbsorptivePotential(Z, pos, box, {14: 0.078, 8: 0.09}), box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tds_detector.txt"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--slices", type=int, default=100)
    ap.add_argument("--scan", type=int, default=16)
    a = ap.parse_args()
    import torch
    import pyslice_amd as ps
    src, box = source(a.grid, a.slices)
    pp = [(box[0, 0] * (i + 0.5) / a.scan, box[1, 1] * (j + 0.5) / a.scan) for i in range(a.scan) for j in range(a.scan)]
    dets = [ps.Detector("haadf", inner=60.0, outer=200.0), ps.Detector("adf", inner=30.0, outer=60.0)]
    calcs = {}
    for tds in (False, True):
        c = ps.MultisliceCalculator(device=0, progress=False, detectors=dets, tds=tds, probe_batch=64)
        c.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=pp, sampling=0.1, slice_thickness=1.0)
        c.run_detectors()                                       # warm-up: kernels loaded, tables made
        calcs[tds] = c
    times = {False: [], True: []}
    for _ in range(a.repeat):
        for tds in (False, True):
            t0 = time.perf_counter()
            res = calcs[tds].run_detectors()
            times[tds].append(time.perf_counter() - t0)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    lines = [f"run_detectors(), {a.scan} x {a.scan} scan, {a.grid}^2 x {a.slices} slices, probe_batch=64, 2 detectors (median of {a.repeat}, s; all runs)",
             f"  tds=False {off:8.3f}   {' '.join(f'{t:.3f}' for t in times[False])}",
             f"  tds=True  {on:8.3f}   {' '.join(f'{t:.3f}' for t in times[True])}",
             f"  ratio {on / off:5.2f}",
             f"  haadf mean: elastic {res.signals[..., 0].mean():.4e}  tds {res.tds[..., 0].mean():.4e}"]
    # the reduction alone, on the work buffer of the TDS engine (64 images), against a copy of as many bytes
    eng = calcs[True]._engine
    P, npix = eng.n_probes, a.grid * a.grid
    _, ms = eng.tds_reduce(a.slices // 2, 200)
    buf = torch.empty(P * npix, dtype=torch.complex64, device="cuda")
    dst = torch.empty_like(buf)
    buf.zero_()
    dst.copy_(buf)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        dst.copy_(buf)
    e1.record()
    torch.cuda.synchronize()
    ms_copy = e0.elapsed_time(e1) / 200
    nbytes = 8.0 * P * npix
    r_red, r_copy = nbytes / (ms * 1e-3) / 1e12, 2.0 * nbytes / (ms_copy * 1e-3) / 1e12
    lines += [f"tds_reduce_kernel alone, {P} images of {a.grid}^2, 2 detectors, 200 launches between two events",
              f"  reduction {ms * 1e3:8.1f} us  {r_red:6.2f} TB/s read",
              f"  device copy of the same buffer {ms_copy * 1e3:8.1f} us  {r_copy:6.2f} TB/s read + written",
              f"  ratio of the rates {r_red / r_copy:5.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

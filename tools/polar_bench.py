"""Polar-detector runs (MultisliceCalculator(polar=...).run_polar()).  One JSON line per case.
--detect-only times msl_polar_detect alone on caller-held random spectra, (rows, 1, n*n) complex64, with R rings x A sectors for
every A given, next to msl_detect with 16 detectors on the same memory, and reports the bytes each reads divided by the time
against 8 TB/s; the wall times include the copy back and the wait (for the kernels alone: rocprofv3 --kernel-trace --stats --
python tools/polar_bench.py --detect-only).
    python tools/polar_bench.py --detect-only [--rows 64] [--n 512 1024] [--rings 128] [--sectors 1 16] [--reps 20]
The scan mode runs a scan x scan raster through run_polar() --runs times in one session and reports the share of the polar pass,
then run_detectors() with 16 detectors on the same scan as the yardstick, with the share of msl_detect.
    python tools/polar_bench.py [--scan 32] [--n 512] [--slices 50] [--frames 1] [--rings 128] [--sectors 16] [--probe-batch 256] [--runs 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyslice_amd as ps  # noqa: E402
from pyslice_amd import _native  # noqa: E402
from pyslice_amd.multislice import wavelength  # noqa: E402
from pyslice_amd.polar_data import bin_counts  # noqa: E402
from pyslice_amd.stem_data import detector_bitmask  # noqa: E402

HBM_PEAK = 8e12
OUTER = 180.0                                              # mrad: inside the 185 mrad the axes of a 0.1 Angstrom sampling reach


def detectors(n):
    """BF, ABF, ADF, DF, four segments of the BF disc, then rings, up to n: intensity signals only"""
    D = ps.Detector
    a = 30.0
    dets = [D("bf", outer=a), D("abf", inner=a / 2, outer=a), D("adf", inner=1.5 * a, outer=150.0), D("df", inner=a, outer=1.5 * a),
            D("seg0", outer=a, azimuth=(0, 90)), D("seg1", outer=a, azimuth=(90, 180)), D("seg2", outer=a, azimuth=(180, 270)),
            D("seg3", outer=a, azimuth=(270, 360))]
    dets += [D(f"ring{i}", inner=5.0 * i, outer=5.0 * i + 5.0) for i in range(16)]
    return dets[:n]


def _timed(fn, reps):
    fn()                                                  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times)


def _line(case, n, rows, nbytes, med, best, **more):
    return json.dumps({"case": case, "grid": n, "rows": rows, **more, "bytes_read": int(nbytes), "ms_median": round(med * 1e3, 4),
                       "ms_min": round(best * 1e3, 4), "GB_per_s": round(nbytes / med / 1e9, 1),
                       "fraction_of_8TBps": round(nbytes / med / HBM_PEAK, 4)})


def detect_only(args):
    import torch
    lam = wavelength(100e3)
    for n in args.n:
        K, rows = n * n, args.rows
        kx = np.fft.fftshift(np.fft.fftfreq(n, 0.1)).astype(np.float32)
        eng = _native.Engine(n, n, 1, 0.1, 0.1, 0.5, lam, 0.0, n_probes=1, n_frames=0)
        g = torch.Generator(device="cuda").manual_seed(1)
        W = torch.view_as_complex(torch.randn((rows, 1, K, 2), dtype=torch.float32, device="cuda", generator=g))
        torch.cuda.synchronize()
        src = (W.data_ptr(), rows, 1, K)
        for A in args.sectors:
            pol = ps.PolarDetector(outer=OUTER, step=OUTER / args.rings, n_azimuthal=A)
            bins = ps.polar_bins(pol, kx, kx, lam)
            counts = bin_counts(bins, pol.n_bins)
            eng.set_polar(bins.reshape(-1), pol.n_bins)
            med, best = _timed(lambda: eng.polar_detect(src=src), args.reps)
            # what the pass must read: the complex values of the pixels in a bin, and their 4-byte indices once per 4 rows
            nbytes = counts.sum() * rows * 8 + counts.sum() * 4 * ((rows + 3) // 4)
            print(_line("polar_detect_only", n, rows, nbytes, med, best, rings=pol.n_rings, sectors=A, bins=pol.n_bins,
                        pixels_in_bins=int(counts.sum()), longest_bin=int(counts.max()), empty_bins=int((counts == 0).sum()),
                        fraction_of_8TBps_whole_rows=round(rows * K * 8 / med / HBM_PEAK, 4)), flush=True)
        dets = detectors(16)
        eng.set_detectors(detector_bitmask(dets, kx, kx, lam).reshape(-1), [d.signal for d in dets], kx, kx)
        med, best = _timed(lambda: eng.detect(src=src), args.reps)
        print(_line("detect_16_detectors", n, rows, rows * K * 8, med, best), flush=True)
        eng.close()
        del W


def _between_waits(eng, name, into):
    fn = getattr(eng, name)

    def call(*a, **k):
        eng.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        eng.synchronize()
        into.append(time.perf_counter() - t0)
        return out
    setattr(eng, name, call)


def scan(args):
    from pyslice_amd.synthetic import synthetic_trajectory
    n = args.n[0]
    tr = synthetic_trajectory(n, args.slices, args.frames, seed=5)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    s = args.scan
    pp = [(x, y) for x in np.linspace(0.25 * lx, 0.75 * lx, s) for y in np.linspace(0.25 * ly, 0.75 * ly, s)]
    steps = len(pp) * args.frames * args.slices
    pol = ps.PolarDetector(outer=OUTER, step=OUTER / args.rings, n_azimuthal=args.sectors[0])
    modes = [("scan_polar", dict(polar=pol), "run_polar", "polar_detect"),
             ("scan_detectors_yardstick", dict(detectors=detectors(16)), "run_detectors", "detect")]
    for run in range(args.runs):
        for case, kw, method, reduction in modes:
            calc = ps.MultisliceCalculator(progress=False, probe_batch=args.probe_batch, frame_batch=args.frame_batch, **kw)
            calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
            eng = calc._engine
            spent = []
            _between_waits(eng, reduction, spent)
            t0 = time.perf_counter()
            res = getattr(calc, method)()
            dt = time.perf_counter() - t0
            print(json.dumps({"case": case, "run": run, "scan": f"{s}x{s}", "grid": n, "slices": args.slices, "frames": args.frames,
                              "probe_batch": eng.n_probes, "frame_batch": eng.frame_batch,
                              "bins": pol.n_bins if "polar" in kw else None, "s_total": round(dt, 3), "slice_steps_per_s": round(steps / dt),
                              "reduction": reduction, "calls": len(spent), "share_pct": round(100.0 * sum(spent) / dt, 3),
                              "ms_per_call": round(1e3 * float(np.median(spent)), 4), "finite": bool(np.isfinite(res.signals).all())}),
                  flush=True)
            calc._engine = None
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--n", type=int, nargs="+", default=None)
    ap.add_argument("--rings", type=int, default=128)
    ap.add_argument("--sectors", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scan", type=int, default=32)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--probe-batch", type=int, default=256)
    ap.add_argument("--frame-batch", type=int, default=None)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if args.detect_only:
        args.n = args.n or [512, 1024]
        args.sectors = args.sectors or [1, 16]
        detect_only(args)
        return
    args.n = args.n or [512]
    args.sectors = args.sectors or [16]
    scan(args)


if __name__ == "__main__":
    main()

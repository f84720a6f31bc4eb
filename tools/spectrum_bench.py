"""Spectrum-image runs (MultisliceCalculator(spectroscopy=...).run_spectrum_image()).  One JSON line per case.
--detect-only times msl_spectrum_detect alone on resident random intensity, (probes, frequencies, n*n) float32, at the given
detector counts, next to ONE msl_tacaw_spectrum call with a byte mask (the path that takes one pass per mask) on the same memory,
and reports the HBM rate of each against 8 TB/s; the wall times include the finishing launch, the copy back and the wait (for the
kernels alone: rocprofv3 --kernel-trace --stats -- python tools/spectrum_bench.py --detect-only).
    python tools/spectrum_bench.py --detect-only [--probes 64] [--frequencies 256] [--n 256] [--detectors 8 16] [--reps 10]
The scan mode runs a scan x scan raster through run_spectrum_image() --runs times in one session and reports the shares of the
potential builds, the slice loop, msl_tacaw and the spectrum pass, then run_detectors() on the same scan as the yardstick.
    python tools/spectrum_bench.py [--scan 16] [--n 512] [--slices 50] [--frames 64] [--window 128] [--probe-batch 64] [--detectors 8] [--runs 2]"""
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
from pyslice_amd.stem_data import detector_bitmask  # noqa: E402

HBM_PEAK = 8e12


def detectors(n):
    """BF, ABF, ADF, four segments of the BF disc, then rings, up to n: intensity signals only"""
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


def detect_only(args):
    import torch
    n, B, F = args.n, args.probes, args.frequencies
    K = n * n
    kx = np.fft.fftshift(np.fft.fftfreq(n, 0.1)).astype(np.float32)
    lam = wavelength(100e3)
    eng = _native.Engine(n, n, 1, 0.1, 0.1, 0.5, lam, 0.0, n_probes=1, n_frames=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    I = torch.rand((B, F, K), dtype=torch.float32, device="cuda", generator=g)
    torch.cuda.synchronize()
    src = (I.data_ptr(), B, F, K)
    nbytes = B * F * K * 4
    for D in args.detectors:
        dets = detectors(D)
        eng.set_detectors(detector_bitmask(dets, kx, kx, lam).reshape(-1), [d.signal for d in dets], kx, kx)
        med, best = _timed(lambda: eng.spectrum_detect(src=src), args.reps)
        print(json.dumps({"case": "spectrum_detect_only", "probes": B, "frequencies": F, "grid": n, "detectors": D, "bytes_read": nbytes,
                          "ms_median": round(med * 1e3, 4), "ms_min": round(best * 1e3, 4), "GB_per_s": round(nbytes / med / 1e9, 1),
                          "fraction_of_8TBps": round(nbytes / med / HBM_PEAK, 3)}), flush=True)
    mask = detectors(1)[0].member(kx, kx, lam)
    med, best = _timed(lambda: eng.tacaw_spectrum(mask, src=src), args.reps)
    print(json.dumps({"case": "tacaw_spectrum_one_mask", "probes": B, "frequencies": F, "grid": n, "bytes_read": nbytes,
                      "ms_median": round(med * 1e3, 4), "ms_min": round(best * 1e3, 4), "GB_per_s": round(nbytes / med / 1e9, 1),
                      "fraction_of_8TBps": round(nbytes / med / HBM_PEAK, 3)}), flush=True)
    eng.close()


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
    import torch
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(args.n, args.slices, args.frames, seed=5)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    s = args.scan
    pp = [(x, y) for x in np.linspace(0.25 * lx, 0.75 * lx, s) for y in np.linspace(0.25 * ly, 0.75 * ly, s)]
    window = (args.window, args.window) if args.window else None
    dets = detectors(args.detectors)
    steps = len(pp) * args.frames * args.slices
    for run in range(args.runs):
        free0 = torch.cuda.mem_get_info()[0]
        calc = ps.MultisliceCalculator(progress=False, spectroscopy=ps.Spectroscopy(dets), probe_batch=args.probe_batch, k_window=window,
                                       frame_batch=args.frame_batch)
        calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        eng = calc._engine
        used = free0 - torch.cuda.mem_get_info()[0]
        spent = {"build": [], "propagate": [], "tacaw": [], "spectrum_detect": []}
        for name, key in (("build_potential", "build"), ("build_potentials", "build"), ("propagate_frame", "propagate"),
                          ("propagate_frames", "propagate"), ("tacaw", "tacaw"), ("spectrum_detect", "spectrum_detect")):
            _between_waits(eng, name, spent[key])
        t0 = time.perf_counter()
        res = calc.run_spectrum_image()
        dt = time.perf_counter() - t0
        print(json.dumps({"case": "scan_spectrum_image", "run": run, "scan": f"{s}x{s}", "grid": args.n, "slices": args.slices, "frames": args.frames,
                          "k_window": args.window, "probe_batch": eng.n_probes, "frame_batch": eng.frame_batch, "detectors": len(dets),
                          "s_total": round(dt, 3), "slice_steps_per_s": round(steps / dt),
                          "calls": {k: len(v) for k, v in spent.items()},
                          "share_pct": {k: round(100.0 * sum(v) / dt, 2) for k, v in spent.items()},
                          "ms_per_call": {k: round(1e3 * float(np.median(v)), 4) if v else None for k, v in spent.items()},
                          "ring_bytes": eng.buffer_bytes(_native.BUF_WAVEFUNCTION), "intensity_bytes": eng.buffer_bytes(_native.BUF_INTENSITY),
                          "device_bytes_after_setup": int(used), "spectra_finite": bool(np.isfinite(res.spectra).all())}), flush=True)
        calc._engine = None
        eng.close()
    calc = ps.MultisliceCalculator(progress=False, detectors=dets, probe_batch=args.probe_batch, k_window=window, frame_batch=args.frame_batch)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    t0 = time.perf_counter()
    st = calc.run_detectors()
    dt = time.perf_counter() - t0
    print(json.dumps({"case": "scan_detectors_yardstick", "scan": f"{s}x{s}", "probe_batch": calc._engine.n_probes, "frame_batch": calc._engine.frame_batch,
                      "s_total": round(dt, 3), "slice_steps_per_s": round(steps / dt), "signals_finite": bool(np.isfinite(st.signals).all())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--frequencies", type=int, default=256)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--detectors", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scan", type=int, default=16)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--probe-batch", type=int, default=64)
    ap.add_argument("--frame-batch", type=int, default=None)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    if args.detect_only:
        args.n = args.n or 256
        args.detectors = args.detectors or [8, 16]
        detect_only(args)
        return
    args.n = args.n or 512
    args.detectors = (args.detectors or [8])[0]
    scan(args)


if __name__ == "__main__":
    main()

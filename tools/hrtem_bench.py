"""HRTEM imaging (MultisliceCalculator(imaging=Imaging(...)).run_images()): the two measurements of DESIGN.md section 4.14, one
JSON line each.
    python tools/hrtem_bench.py --pass-only [--images 256] [--n 1024] [--reps 10]
        msl_image_add alone (count = 1, one defocus, Cs + defocus + aperture) on --images resident spectra: wall time per call
        between two waits.  For the split into lens / inverse transform / accumulate run it under a kernel trace of its own,
        rocprofv3 --kernel-trace --stats -- python tools/hrtem_bench.py --pass-only: the yardstick is the two fft2_inplace launches
        inside the same trace (by bytes per pixel and image the lens moves 16 B, the accumulation 8 B + the amortised accumulator,
        the transform pair 32 B).
    python tools/hrtem_bench.py --end-to-end [--n 1024] [--slices 200] [--frames 64] [--runs 2] [--series 21]
        plane wave, one probe: run_images() with one defocus against run() with output="device" on the same trajectory, --runs
        times each in turn, then run_images() with a focal series of --series values (reported, not bounded)."""
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


def lens(series=(-430.0,)):
    """Cs = 1 mm near Scherzer defocus at 100 kV behind a 25 mrad objective aperture"""
    return ps.Imaging(aberrations=ps.Aberrations(Cs=1.0e7), aperture_mrad=25.0, defocus_series=tuple(series))


def pass_only(args):
    import torch
    n, B = args.n, args.images
    lam = wavelength(100e3)
    eng = _native.Engine(n, n, 1, 0.1, 0.1, 0.5, lam, 0.0, n_probes=B, n_frames=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn((B, 1, n * n), dtype=torch.complex64, device="cuda", generator=g)
    torch.cuda.synchronize()
    im = lens()
    kw = dict(polar=im.polar(), aperture_k=im.aperture_k(lam), src=(W.data_ptr(), B, 1, n * n))
    eng.image_reset(B)
    eng.image_add(0, 1, **kw)                              # warm-up
    eng.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.image_add(0, 1, **kw)                          # lens + two transform launches + accumulate, queued: the wait is ours
        eng.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    nbytes = B * n * n * (16 + 32 + 8 + 16)                # lens, transform pair, |psi|^2 read, accumulator read + write
    print(json.dumps({"case": "image_pass_only", "images": B, "grid": n, "count": 1, "reps": args.reps, "ms_median": round(dt * 1e3, 4),
                      "ms_min": round(min(times) * 1e3, 4), "bytes_moved": nbytes, "GB_per_s": round(nbytes / dt / 1e9, 1)}), flush=True)
    eng.close()


def end_to_end(args):
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(args.n, args.slices, args.frames, seed=5)
    steps = args.frames * args.slices
    out = {"case": "hrtem_end_to_end", "grid": args.n, "slices": args.slices, "frames": args.frames, "probes": 1}

    def run_plain():
        calc = ps.MultisliceCalculator(progress=False, output="device")
        calc.setup(tr, aperture=0.0, voltage_eV=100e3)
        t0 = time.perf_counter()
        calc.run()                                         # (ends with a wait for the stream)
        dt = time.perf_counter() - t0
        fb = calc._engine.frame_batch
        calc._engine.close()
        return dt, fb

    def run_images(series):
        calc = ps.MultisliceCalculator(progress=False, imaging=lens(series))
        calc.setup(tr, aperture=0.0, voltage_eV=100e3)
        t0 = time.perf_counter()
        data = calc.run_images()                           # (ends with the download of the images)
        dt = time.perf_counter() - t0
        fb = calc._engine.frame_batch
        calc._engine.close()
        return dt, fb, bool(np.isfinite(data.intensity).all())
    run_plain()                                            # warm-up of both paths
    run_images((-430.0,))
    plain, images = [], []
    for _ in range(args.runs):
        dt, fb = run_plain()
        plain.append(dt)
        dt, fbi, ok = run_images((-430.0,))
        images.append(dt)
    out.update(frame_batch_run=fb, frame_batch_images=fbi, run_device_s=[round(v, 4) for v in plain], run_images_s=[round(v, 4) for v in images],
               run_slice_steps_per_s=round(steps / min(plain)), images_slice_steps_per_s=round(steps / min(images)),
               images_over_run=round(min(images) / min(plain), 4), images_finite=ok)
    series = np.linspace(-800.0, 0.0, args.series)
    dt, _, ok = run_images(series)
    out.update(series=args.series, run_images_series_s=round(dt, 4), series_over_run=round(dt / min(plain), 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass-only", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--series", type=int, default=21)
    args = ap.parse_args()
    if not (args.pass_only or args.end_to_end):
        ap.error("give --pass-only or --end-to-end")
    if args.pass_only:
        pass_only(args)
    if args.end_to_end:
        end_to_end(args)


if __name__ == "__main__":
    main()

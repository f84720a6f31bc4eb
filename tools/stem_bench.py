"""STEM detector runs (MultisliceCalculator(detectors=...).run_detectors()): slice-steps/s of a scan streamed over probe batches,
the device time of the detector pass (msl_detect) and its share of the run, and the engine's device memory.  One JSON line per
probe batch.  --detect-only times msl_detect alone on resident images and reports its HBM rate against 8 TB/s.
--diffraction BX,BY adds the diffraction-pattern leg: with --detect-only msl_diffract alone on the same resident images, otherwise
the scan through run_diffraction() (with --detectors 0 the patterns alone, else patterns and detectors in one pass).
    python tools/stem_bench.py [--scan 64] [--n 1024] [--slices 200] [--frames 1] [--probe-batch 64 256] [--detectors 8] [--diffraction 8,8]
    python tools/stem_bench.py --detect-only [--images 256] [--n 1024] [--detectors 8] [--reps 20] [--diffraction 8,8]
--split (with --diffraction) adds the elastic / thermal-diffuse split: with --detect-only the coherent accumulation pass
(msl_coherent_add, count = 1) alone on the same resident images, next to msl_diffract for a kernel trace of both in one run
(--diffraction 1,1 is the yardstick of equal traffic per byte); otherwise the scan through run_diffraction() with
Diffraction(split=True), whose JSON line also carries the time of the potential builds and of the coherent pass.
--aberrations runs the scan with an aberrated probe (all fourteen terms non-zero) for an A/B against the plain run in one session.
--probes-only rebuilds --images probes, plain and aberrated in turn, --reps times each: the two probe kernels side by side for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/stem_bench.py --probes-only); the wall times it prints include the
inverse FFT, the transposed copy and the synchronisation.
    python tools/stem_bench.py --probes-only [--images 256] [--n 1024] [--reps 20]"""
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
    """BF, ABF, ADF, HAADF (|Psi|), four DPC segments of the BF disc, then CoM x / y, ... up to n"""
    D = ps.Detector
    a = 30.0
    dets = [D("bf", outer=a), D("abf", inner=a / 2, outer=a), D("adf", inner=1.5 * a, outer=150.0), D("haadf", inner=1.5 * a, signal="amplitude"),
            D("dpc0", outer=a, azimuth=(0, 90)), D("dpc1", outer=a, azimuth=(90, 180)), D("dpc2", outer=a, azimuth=(180, 270)),
            D("dpc3", outer=a, azimuth=(270, 360)), D("comx", signal="com_x"), D("comy", signal="com_y")]
    dets += [D(f"ring{i}", inner=10.0 * i, outer=10.0 * i + 10.0) for i in range(16)]
    return dets[:n]


def all_aberrations():
    """every term non-zero: Cs = 1 mm (344 rad at the edge of the 30 mrad aperture at 100 kV), -600 A of defocus (-46 rad), the
    others 0.6 - 3 rad each"""
    return ps.Aberrations(defocus=-600.0, astigmatism=40.0, astigmatism_angle=0.3, coma=900.0, coma_angle=1.1, C23=700.0, phi23=0.2,
                          Cs=1e7, C32=2e4, phi32=0.5, C34=2e4, phi34=0.1, C41=8e5, phi41=2.0, C43=8e5, phi43=0.4, C45=8e5, phi45=0.3,
                          C5=5e7, C52=3e7, phi52=1.0, C54=3e7, phi54=0.2, C56=3e7, phi56=0.1)


def probes_only(args):
    n, P = args.n, args.images
    eng = _native.Engine(n, n, 1, 0.1, 0.1, 0.5, wavelength(100e3), 0.0, n_probes=P, n_frames=0)
    xy = np.random.default_rng(3).random((P, 2)) * n * 0.1
    ab = all_aberrations()
    times = {"plain": [], "aberrated": []}
    for rep in range(args.reps + 1):
        for name, a in (("plain", None), ("aberrated", ab)):
            eng.set_aberrations(a)
            t0 = time.perf_counter()
            eng.set_probes(30.0, xy)                      # synchronous
            if rep:                                       # (the first round is the warm-up)
                times[name].append(time.perf_counter() - t0)
    print(json.dumps({"case": "probes_only", "probes": P, "grid": n, "reps": args.reps,
                      "set_probes_ms_median": {k: round(1e3 * float(np.median(v)), 4) for k, v in times.items()}}), flush=True)
    eng.close()


def detect_only(args):
    import torch
    n, B = args.n, args.images
    dets = detectors(args.detectors)
    eng = _native.Engine(n, n, 1, 0.1, 0.1, 0.5, wavelength(100e3), 0.0, n_probes=1, n_frames=0)
    kx = np.fft.fftshift(np.fft.fftfreq(n, 0.1)).astype(np.float32)
    eng.set_detectors(detector_bitmask(dets, kx, kx, wavelength(100e3)).reshape(-1), [d.signal for d in dets], kx, kx)
    g = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn((B, 1, n * n), dtype=torch.complex64, device="cuda", generator=g)
    torch.cuda.synchronize()
    src = (W.data_ptr(), B, 1, n * n)
    eng.detect(src=src)                                   # warm-up
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.detect(src=src)                               # one launch + the finishing launch + 8 B x B x D back, synchronous
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    nbytes = B * n * n * 8
    print(json.dumps({"case": "detect_only", "images": B, "grid": n, "detectors": len(dets), "ms_median": round(dt * 1e3, 4),
                      "ms_min": round(min(times) * 1e3, 4), "GB_per_s": round(nbytes / dt / 1e9, 1),
                      "fraction_of_8TBps": round(nbytes / dt / HBM_PEAK, 3)}), flush=True)
    if args.diffraction:
        bx, by = args.diffraction
        dsrc = (W.data_ptr(), B, 1, n, n)
        eng.diffract(bin=(bx, by), src=dsrc)              # warm-up (allocates the staging array)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.diffract(bin=(bx, by), src=dsrc)          # one launch + 8 B x B x mx x my back, synchronous
            times.append(time.perf_counter() - t0)
        dt = float(np.median(times))
        print(json.dumps({"case": "diffract_only", "images": B, "grid": n, "bin": [bx, by], "ms_median_with_copy": round(dt * 1e3, 4),
                          "ms_min_with_copy": round(min(times) * 1e3, 4), "bytes_read": nbytes, "bytes_copied_back": B * (n // bx) * (n // by) * 8}),
              flush=True)
    if args.diffraction and args.split:
        eng.coherent_reset(B)                             # (B, pitch) float64 complex: 16 B per pixel
        eng.coherent_add(src=src)                         # warm-up
        eng.synchronize()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.coherent_add(src=src)                     # one launch, queued: the wait is ours
            eng.synchronize()
            times.append(time.perf_counter() - t0)
        dt = float(np.median(times))
        print(json.dumps({"case": "coherent_add_only", "images": B, "grid": n, "count": 1, "ms_median": round(dt * 1e3, 4),
                          "ms_min": round(min(times) * 1e3, 4), "bytes_moved": 5 * nbytes, "GB_per_s": round(5 * nbytes / dt / 1e9, 1)}), flush=True)
    eng.close()


def scan(args, pb):
    import torch
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(args.n, args.slices, args.frames, seed=5)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
    s = args.scan
    pp = [(x, y) for x in np.linspace(0.25 * lx, 0.75 * lx, s) for y in np.linspace(0.25 * ly, 0.75 * ly, s)]
    free0 = torch.cuda.mem_get_info()[0]
    if args.diffraction:
        scan_diffraction(args, pb, tr, pp, free0)
        return
    calc = ps.MultisliceCalculator(progress=False, detectors=detectors(args.detectors), probe_batch=pb,
                                   aberrations=all_aberrations() if args.aberrations else None)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    eng = calc._engine
    used = free0 - torch.cuda.mem_get_info()[0]
    buf = {name: eng.buffer_bytes(getattr(_native, "BUF_" + name)) for name in ("PROBES", "EXIT", "TRANSMISSION", "WAVEFUNCTION")}
    # time every detector pass on its own: wait for the slice loop, then the (synchronous) msl_detect
    spent = []
    plain_detect = eng.detect

    def timed_detect(*a, **k):
        eng.synchronize()
        t0 = time.perf_counter()
        out = plain_detect(*a, **k)
        spent.append(time.perf_counter() - t0)
        return out
    eng.detect = timed_detect
    t0 = time.perf_counter()
    st = calc.run_detectors()
    dt = time.perf_counter() - t0
    steps = len(pp) * args.frames * args.slices
    print(json.dumps({"case": "scan", "scan": f"{s}x{s}", "grid": args.n, "slices": args.slices, "frames": args.frames,
                      "probe_batch": eng.n_probes, "frame_batch": eng.frame_batch, "detectors": len(st.detectors),
                      "aberrations": bool(args.aberrations),
                      "s_total": round(dt, 3), "slice_steps_per_s": round(steps / dt),
                      "detect_ms_per_batch": round(1e3 * float(np.median(spent)), 4), "detect_share_pct": round(100.0 * sum(spent) / dt, 3),
                      "engine_buffer_bytes": buf, "device_bytes_after_setup": int(used),
                      "signals_finite": bool(np.isfinite(st.signals).all())}), flush=True)
    calc._engine = None
    eng.close()


def scan_diffraction(args, pb, tr, pp, free0):
    """the scan through run_diffraction(): slice-steps/s, the synchronous msl_diffract per batch, the host accumulate per batch"""
    import torch
    dets = detectors(args.detectors) if args.detectors > 0 else None
    calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(bin=args.diffraction, split=args.split), detectors=dets, probe_batch=pb,
                                   aberrations=all_aberrations() if args.aberrations else None)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    eng = calc._engine
    used = free0 - torch.cuda.mem_get_info()[0]
    spent = []
    plain = eng.diffract

    def timed(*a, **k):
        eng.synchronize()
        t0 = time.perf_counter()
        out = plain(*a, **k)
        spent.append(time.perf_counter() - t0)
        return out
    eng.diffract = timed
    # the potential builds and the coherent pass, each between two waits of its own (a handful per probe batch)
    built, added = [], []

    def between_waits(fn, into):
        def call(*a, **k):
            eng.synchronize()
            t1 = time.perf_counter()
            out = fn(*a, **k)
            eng.synchronize()
            into.append(time.perf_counter() - t1)
            return out
        return call
    eng.build_potential = between_waits(eng.build_potential, built)
    eng.build_potentials = between_waits(eng.build_potentials, built)
    eng.coherent_add = between_waits(eng.coherent_add, added)
    t0 = time.perf_counter()
    dd = calc.run_diffraction()
    dt = time.perf_counter() - t0
    steps = len(pp) * args.frames * args.slices
    block = np.ones((eng.n_probes,) + dd.intensity.shape[1:])
    acc = []
    for i in range(5):                                     # the += of one batch into the host result, on the result itself
        t1 = time.perf_counter()
        dd.intensity[:eng.n_probes] += block
        acc.append(time.perf_counter() - t1)
    print(json.dumps({"case": "scan_diffraction", "scan": f"{args.scan}x{args.scan}", "grid": args.n, "slices": args.slices, "frames": args.frames,
                      "probe_batch": eng.n_probes, "frame_batch": eng.frame_batch, "bin": list(args.diffraction), "aberrations": bool(args.aberrations),
                      "detectors": 0 if dets is None else len(dets), "pattern_shape": list(dd.intensity.shape),
                      "s_total": round(dt, 3), "slice_steps_per_s": round(steps / dt),
                      "diffract_ms_per_batch": round(1e3 * float(np.median(spent)), 4), "diffract_share_pct": round(100.0 * sum(spent) / dt, 3),
                      "accumulate_ms_per_batch": round(1e3 * float(np.median(acc)), 4), "host_result_bytes": int(dd.intensity.nbytes),
                      "split": bool(args.split), "potential_builds": len(built), "potential_ms_per_build": round(1e3 * float(np.median(built)), 3),
                      "potential_share_pct": round(100.0 * sum(built) / dt, 3), "coherent_add_calls": len(added),
                      "coherent_add_ms_per_call": round(1e3 * float(np.median(added)), 4) if added else None,
                      "coherent_add_share_pct": round(100.0 * sum(added) / dt, 3),
                      "device_bytes_after_setup": int(used)}), flush=True)
    calc._engine = None
    eng.close()


def _bin(text):
    bx, by = (int(v) for v in text.split(","))
    return bx, by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--scan", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=200)
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--probe-batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--detectors", type=int, default=8)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--diffraction", type=_bin, default=None, metavar="BX,BY")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--aberrations", action="store_true")
    ap.add_argument("--probes-only", action="store_true")
    args = ap.parse_args()
    if args.split and not args.diffraction:
        ap.error("--split needs --diffraction BX,BY")
    if args.probes_only:
        probes_only(args)
        return
    if args.detect_only:
        detect_only(args)
        return
    for pb in args.probe_batch:
        scan(args, pb)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""PRISM measurements: the synthesis pass alone, and run_detectors() with and without prism.

    python tools/prism_bench.py --pass-only  [--n 512] [--kv 200] [--mrad 30] [--probes 64] [--calls 20] [--crop] [--diffract]
    python tools/prism_bench.py --end-to-end [--n 512] [--slices 100] [--scan 32] [--frames 2] [--kv 200] [--mrad 30] [--crop]

--crop: the probes on the cropped (n / f) grid (msl_smatrix_probes_cropped, Prism(f, crop=True)) next to the uncropped ones.
--diffract: the pass-only step also reduces every call's slot with msl_diffract (the probe stage of a 4D-STEM scan).

Every GPU step runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the
tool (nothing more is started on the device).  One JSON line per step.  For kernel times run the pass-only step under a kernel
trace of its own (tools/collect_kernel_profile.sh style: rocprofv3 --kernel-trace --stats -- python tools/prism_bench.py --child pass ...).
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def child_pass(a):
    """smatrix_probes alone on a resident S-matrix: wall time per call over `calls` queued calls, against the byte model"""
    import numpy as np
    from pyslice_amd import _native, prism
    from pyslice_amd.multislice import interaction_sigma, wavelength
    n, eV, f = a.n, a.kv * 1e3, (a.f, a.f)
    d = 0.1
    eng = _native.Engine(n, n, 2, d, d, 0.5, wavelength(eV), interaction_sigma(eV), n_probes=a.probes, n_frames=1)
    rng = np.random.default_rng(0)
    eng.upload_potential((rng.random((2, n, n)) * 50.0).astype(np.float32))
    Bm = eng.smatrix_begin(f, a.mrad)
    eng.smatrix_build()
    side = int(np.ceil(np.sqrt(a.probes)))
    gx, gy = np.meshgrid(np.linspace(0.2, 0.8, side) * n * d, np.linspace(0.2, 0.8, side) * n * d)
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1)[:a.probes]
    crop = a.crop and a.f > 1
    res = _native.Engine(n // a.f, n // a.f, 1, d, d, 0.5, wavelength(eV), interaction_sigma(eV), n_probes=a.probes, n_frames=1) if crop else eng

    def call():
        if crop:
            eng.smatrix_probes_cropped(res, xy, 0)
        else:
            eng.smatrix_probes(xy, 0)
        if a.diffract:
            res.diffract(0, 1)
    for _ in range(3):
        call()
    res.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        call()
    res.synchronize()
    ms = (time.perf_counter() - t0) / a.calls * 1e3
    G = 16 if a.probes > 8 else 8
    groups = -(-a.probes // G)
    # pixels touched: per group the union of its windows, bounded by groups x the grid; the model takes the windows as disjoint
    touched = min(n * n, G * (n // a.f) * (n // a.f)) * groups
    m = n // a.f if crop else n                                  # the grid the waves are written and transformed on
    read, written = 8.0 * Bm * touched, 8.0 * a.probes * m * m * 2
    print(json.dumps({"step": "pass", "crop": bool(crop), "diffract": bool(a.diffract), "n": n, "kV": a.kv, "mrad": a.mrad, "f": a.f, "probes": a.probes, "beams": Bm, "G": G,
                      "ms_per_call_wall": round(ms, 4), "model_read_GB": round(read / 1e9, 3), "model_written_GB": round(written / 1e9, 3),
                      "model_fraction_of_hbm_peak_wall": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}))
    if crop:
        res.close()
    eng.close()


def child_e2e(a):
    """run_detectors() of one scan: mode = multislice | prism1 | prismF | prismFcrop"""
    import numpy as np
    import pyslice_amd as ps
    from pyslice_amd.prism import Prism
    from pyslice_amd.stem_data import Detector
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(a.n, a.slices, a.frames, density=0.05, seed=1)
    L = tr.box_matrix[0, 0]
    g = np.linspace(0.1, 0.9, a.scan) * L
    pp = [(float(x), float(y)) for x in g for y in g]
    pr = {"multislice": None, "prism1": Prism(1), "prismF": Prism(a.f), "prismFcrop": Prism(a.f, crop=True)}[a.mode]
    calc = ps.MultisliceCalculator(device=0, progress=False, detectors=[Detector("adf", inner=60.0, outer=200.0)], prism=pr)
    calc.setup(tr, aperture=a.mrad, voltage_eV=a.kv * 1e3, probe_positions=pp)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        st = calc.run_detectors()
        times.append(time.perf_counter() - t0)
    ctr = calc._source_engine().counters()                       # (crop: the beam engine runs the slice loops)
    print(json.dumps({"step": "e2e", "mode": a.mode, "n": a.n, "slices": a.slices, "probes": len(pp), "frames": a.frames, "f": a.f,
                      "beams": getattr(calc, "_prism_Bm", 0), "probe_batch": calc.probe_batch, "seconds": [round(t, 4) for t in times],
                      "slice_steps_total": int(ctr["slice_steps"]), "adf_mean": float(np.mean(st.signals))}))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"step": "failed", "cmd": args, "exit": rc}))
        sys.exit(rc if 0 < rc < 256 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass-only", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--child", choices=["pass", "e2e"])
    ap.add_argument("--mode", default="multislice")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--kv", type=float, default=200.0)
    ap.add_argument("--mrad", type=float, default=30.0)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--f", type=int, default=4)
    ap.add_argument("--slices", type=int, default=100)
    ap.add_argument("--scan", type=int, default=32)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--crop", action="store_true", help="also the probes on the cropped grid")
    ap.add_argument("--diffract", action="store_true", help="pass-only: msl_diffract of every call's slot as well")
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    a = ap.parse_args()
    if a.child == "pass":
        return child_pass(a)
    if a.child == "e2e":
        return child_e2e(a)
    common = ["--n", str(a.n), "--kv", str(a.kv), "--mrad", str(a.mrad)]
    if a.pass_only:
        extra = ["--diffract"] if a.diffract else []
        for f in (1, a.f):
            run_child(["--child", "pass", "--f", str(f), "--probes", str(a.probes), "--calls", str(a.calls)] + extra + common, a.limit)
        if a.crop:
            run_child(["--child", "pass", "--crop", "--f", str(a.f), "--probes", str(a.probes), "--calls", str(a.calls)] + extra + common, a.limit)
    if a.end_to_end:
        for mode in ("multislice", "prismF", "prism1") + (("prismFcrop",) if a.crop else ()):
            run_child(["--child", "e2e", "--mode", mode, "--f", str(a.f), "--slices", str(a.slices), "--scan", str(a.scan),
                       "--frames", str(a.frames)] + common, a.limit)
    if not (a.pass_only or a.end_to_end):
        ap.error("give --pass-only and / or --end-to-end")


if __name__ == "__main__":
    main()

"""Cost of the thickness series of the probe-batch modes (MultisliceCalculator(thickness=...), msl_set_layer_reduce).

    python tools/thickness_bench.py [--scan 64] [--n 1024] [--slices 200] [--probe-batch 64] [--entries 3 20] [--reps 3] [--plain-only]

1. The scan: run_detectors() of a scan x scan raster (3 detectors) with thickness=None, 3 and 20 entries -- seconds per scan, the
   overhead in per cent, the added time per entry and probe batch, device bytes of the mode after setup().
2. The same-session yardsticks, on one engine of one probe batch: the tap (slice loop with msl_set_layers on 3 layers minus the
   plain loop, per layer -- what tools/layers_bench.py measures), and the stand-alone msl_detect / msl_polar_detect / msl_diffract
   passes on the exit block (tools/stem_bench.py, tools/polar_bench.py), each with its download.
   Claim: added time per entry and probe batch <= 1.1 x (tap + detect pass), the passes the scan of part 1 runs.
--plain-only: part 1 with thickness=None alone (this is what a checkout of an earlier commit can run, for the no-regression guard).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyslice_amd as ps  # noqa: E402
from pyslice_amd import _native  # noqa: E402
from pyslice_amd.multislice import interaction_sigma, wavelength  # noqa: E402
from pyslice_amd.synthetic import synthetic_trajectory  # noqa: E402


def detectors():
    return [ps.Detector("bf", outer=10.0), ps.Detector("abf", inner=10.0, outer=20.0), ps.Detector("adf", inner=40.0, outer=150.0)]


def entries(n, nz):
    """n thickness entries spread evenly over the stack, the exit last"""
    return sorted({int(round((i + 1) * nz / n)) - 1 for i in range(n - 1)} - {nz - 1})


def scan(args, tr, pp, n_entries):
    kw = {} if n_entries == 0 else dict(thickness=entries(n_entries, args.slices))
    calc = ps.MultisliceCalculator(progress=False, detectors=detectors(), probe_batch=args.probe_batch, frame_batch=1, **kw)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    eng = calc._engine
    mode = {k: eng.layer_reduce_bytes(w) for k, w in (("block", 0), ("tap", 1), ("staging", 2))} if n_entries else {}
    calc.run_detectors()                                   # warm-up (clocks, code objects, the phase tables)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = calc.run_detectors()
        times.append(time.perf_counter() - t0)
    out = dict(case="scan", entries=n_entries, L=1 if n_entries == 0 else len(res.layer), probes=len(pp), probe_batch=calc.probe_batch,
               seconds=min(times), seconds_all=[round(t, 4) for t in times], mode_bytes=mode, shape=list(res.signals.shape))
    print(json.dumps(out), flush=True)
    return out


def timed(fn, reps, sync):
    fn(); sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def yardsticks(args):
    n, nz, P = args.n, args.slices, args.probe_batch
    eng = _native.Engine(n, n, nz, 0.1, 0.1, 0.5, wavelength(100e3), interaction_sigma(100e3), n_probes=P, n_frames=1)
    V = (np.random.default_rng(3).random((nz, n, n), dtype=np.float32) * 2.0).astype(np.float32)
    eng.set_probes(30.0, np.column_stack([np.linspace(10, 90, P), np.full(P, 50.0)]))
    eng.upload_potential(V)
    kx = np.fft.fftshift(np.fft.fftfreq(n, 0.1)).astype(np.float32)
    from pyslice_amd.polar_data import polar_bins
    from pyslice_amd.stem_data import detector_bitmask
    dets, pol = detectors(), ps.PolarDetector(outer=150.0, step=2.0, n_azimuthal=4)
    eng.set_detectors(detector_bitmask(dets, kx, kx, wavelength(100e3)).reshape(-1), [d.signal for d in dets], kx, kx)
    eng.set_polar(polar_bins(pol, kx, kx, wavelength(100e3)).reshape(-1), pol.n_bins)
    reps = max(3, args.reps)
    loop = timed(lambda: eng.propagate_frame(0), reps, eng.synchronize)
    layers = entries(4, nz)
    eng.set_layers(layers)
    tapped = timed(lambda: eng.propagate_frame(0), reps, eng.synchronize)
    eng.set_layers([])
    eng.propagate_frame(0)
    out = dict(case="yardsticks", images=P, loop_ms=1e3 * loop, tap_ms=1e3 * (tapped - loop) / len(layers),
               detect_ms=1e3 * timed(lambda: eng.detect(0, 1), reps, eng.synchronize),
               polar_ms=1e3 * timed(lambda: eng.polar_detect(0, 1), reps, eng.synchronize),
               diffract_ms=1e3 * timed(lambda: eng.diffract(0, 1, bin=(8, 8)), reps, eng.synchronize))
    # the same engine in the reduce mode: the loop with 4 entries, every reduction on
    eng.set_layer_reduce(layers, _native.LR_DETECT | _native.LR_POLAR | _native.LR_DIFFRACT, bin=(8, 8))

    def seq():
        eng.propagate_frame(0)
        eng.layer_fetch(1)
    exit_ms = out["detect_ms"] + out["polar_ms"] + out["diffract_ms"]         # (the exit layer's passes, without a tap)
    out["all_reductions_entry_ms"] = (1e3 * (timed(seq, reps, eng.synchronize) - loop) - exit_ms) / len(layers)
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=200)
    ap.add_argument("--probe-batch", type=int, default=64)
    ap.add_argument("--entries", type=int, nargs="*", default=[3, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    tr = synthetic_trajectory(args.n, args.slices, 1, density=0.01, seed=2)
    lx = tr.box_matrix[0, 0]
    g = np.linspace(0.2 * lx, 0.8 * lx, args.scan)
    pp = [(float(x), float(y)) for x in g for y in g]
    plain = scan(args, tr, pp, 0)
    if args.plain_only:
        return
    yard = yardsticks(args)
    batches = -(-len(pp) // plain["probe_batch"])
    runs = [scan(args, tr, pp, n) for n in args.entries]
    for r in runs:
        added = 1e3 * (r["seconds"] - plain["seconds"]) / batches / (r["L"] - 1)
        print(json.dumps(dict(case="summary", entries=r["L"], overhead_percent=100.0 * (r["seconds"] / plain["seconds"] - 1.0),
                              added_ms_per_entry_and_batch=added, yardstick_ms=yard["tap_ms"] + yard["detect_ms"],
                              within_claim=bool(added <= 1.1 * (yard["tap_ms"] + yard["detect_ms"])),
                              mode_bytes=sum(r["mode_bytes"].values()))), flush=True)


if __name__ == "__main__":
    main()

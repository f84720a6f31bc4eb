"""Cost of the thickness series (msl_set_layers): slice loop + exit FFT of 64 probes x 1024^2 x 200 slices x 4 frames (one launch
sequence of 256 images), without layers and with layers = [49, 99, 149].  Prints one JSON line per case and the tap time per layer
per 256 images; the launch_timing pass shows that the slice-loop kernels themselves do not change.
    python tools/layers_bench.py [--reps 5] [--n 1024] [--slices 200] [--probes 64] [--frames 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyslice_amd import _native  # noqa: E402
from pyslice_amd.multislice import interaction_sigma, wavelength  # noqa: E402


def run(args, layers, timing):
    n, nz, P, B = args.n, args.slices, args.probes, args.frames
    eng = _native.Engine(n, n, nz, 0.1, 0.1, 0.5, wavelength(100e3), interaction_sigma(100e3), n_probes=P, n_frames=B,
                         frame_batch=B, launch_timing=timing)
    rng = np.random.default_rng(3)
    V = (rng.random((nz, n, n), dtype=np.float32) * 2.0).astype(np.float32)
    eng.set_probes(30.0, np.column_stack([np.linspace(10, 90, P), np.full(P, 50.0)]))
    for b in range(B):
        eng.select_batch_slot(b)
        eng.upload_potential(V)
    if layers:
        eng.set_layers(layers)
    eng.propagate_frames(0, B)                    # warm-up (clocks, code objects)
    eng.synchronize()
    eng.reset_counters()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        eng.propagate_frames(0, B)
    eng.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    c = eng.counters()
    eng.close()
    return dt, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=200)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--frames", type=int, default=4)
    args = ap.parse_args()
    layers = [args.slices // 4 - 1, args.slices // 2 - 1, 3 * args.slices // 4 - 1]
    steps = args.probes * args.slices * args.frames
    images = args.probes * args.frames
    res = {}
    for name, lay in (("plain", []), ("layers", layers)):
        dt, _ = run(args, lay, False)
        _, c = run(args, lay, True)
        res[name] = dt
        print(json.dumps({"case": name, "layers": lay, "grid": args.n, "slices": args.slices, "probes": args.probes,
                          "frames": args.frames, "ms_per_sequence": round(dt * 1e3, 3), "slice_steps_per_s": round(steps / dt),
                          "ms_slice_kernels_per_sequence": round(c["ms_slice_kernels"] / args.reps, 3),
                          "algorithmic_bytes_per_sequence": int(c["algorithmic_bytes"] // args.reps)}), flush=True)
    tap = (res["layers"] - res["plain"]) / len(layers) * 1e3 * 256.0 / images
    print(json.dumps({"tap_ms_per_layer_per_256_images": round(tap, 3),
                      "overhead_pct": round(100.0 * (res["layers"] / res["plain"] - 1.0), 2)}), flush=True)


if __name__ == "__main__":
    main()

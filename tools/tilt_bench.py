"""Cost of one tilt change: the propagator tables written on the device (msl_set_tilt) against the host fill and synchronous copies
(msl_set_beam on a handle that was never tilted, the only path before msl_set_tilt existed), and a 16-tilt precession
run_diffraction() against 16 separate single-tilt runs.

    python tools/tilt_bench.py [--out profiles/tilt_tables.txt] [--repeat 20]

Both table paths are timed to completion (msl_synchronize) on a handle that is otherwise idle, at (0, 0): that writes every table,
the convolution filters included (a non-zero tangent along a convolution axis skips its filter, which no pass could read).

It also times the slice loop of a grid whose axes are zero-padded convolutions with and without a tilt: a tilt along such an axis runs
on the two-pass loop, and this is what that costs per slice-step."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EV = 100e3


def table_times(nx, ny, repeat):
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    lam, sig = wavelength(EV), interaction_sigma(EV)
    eng = _native.Engine(nx, ny, 4, 0.1, 0.1, 2.0, lam, sig, n_probes=1)
    try:
        out = {}
        for name, call in (("host fill + copies (msl_set_beam)", lambda: eng.set_beam(lam, sig, 2.0)),
                           ("device (msl_set_tilt)", lambda: eng.set_tilt(0.0, 0.0))):
            call()
            eng.synchronize()
            ts = []
            for _ in range(repeat):
                t0 = time.perf_counter()
                call()
                eng.synchronize()
                ts.append(time.perf_counter() - t0)
            out[name] = (float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3)
        return out
    finally:
        eng.close()


def loop_times(nx, ny, nz, P, repeat):
    """ms per slice loop (msl_propagate to completion) on one handle: untilted through the device tables (one-pass loop), and tilted
    along both axes (the two-pass loop where an axis is a convolution)"""
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    eng = _native.Engine(nx, ny, nz, 0.1, 0.1, 2.0, wavelength(EV), interaction_sigma(EV), n_probes=P)
    try:
        eng.set_probes(30.0, np.asarray([(1.0 + 0.5 * i, 2.0 + 0.25 * i) for i in range(P)]))
        eng.upload_potential(np.zeros((nz, nx, ny), dtype=np.float32))
        out = []
        for tan in ((0.0, 0.0), (0.05, -0.03)):
            eng.set_tilt(*tan)
            eng.propagate()
            eng.synchronize()
            ts = []
            for _ in range(repeat):
                t0 = time.perf_counter()
                eng.propagate()
                eng.synchronize()
                ts.append(time.perf_counter() - t0)
            out.append(float(np.median(ts)) * 1e3)
        return out
    finally:
        eng.close()


def precession_times(nx, ny, n_tilts):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(nx, 8, 1, ny=ny, slice_thickness=2.0, density=0.03, seed=1)
    pp = [(1.0 + 0.7 * i, 2.0 + 0.3 * i) for i in range(4)]
    pre = ps.Precession(10.0, n_tilts)

    def run(**kw):
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(), **kw)
        calc.setup(tr, aperture=30.0, voltage_eV=EV, probe_positions=pp, slice_thickness=2.0)
        t0 = time.perf_counter()
        calc.run_diffraction()
        return time.perf_counter() - t0
    run(precession=pre)                                                      # (warm-up: kernels loaded, tables made)
    t0 = time.perf_counter()
    inner = run(precession=pre)
    one = time.perf_counter() - t0
    t0 = time.perf_counter()
    for t in pre.tilts():
        run(tilt=t)
    sep = time.perf_counter() - t0
    return one, inner, sep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tilt_tables.txt"))
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    lines = ["tilt change: every propagator table of both axes, to completion, one idle handle (median / min ms over %d calls)" % a.repeat]
    for nx, ny in ((501, 501), (1024, 1024), (2047, 1500)):
        for name, (med, lo) in table_times(nx, ny, a.repeat).items():
            lines.append(f"  {nx} x {ny}  {name:36s} {med:9.3f} / {lo:9.3f}")
    lines.append("slice loop, ms per msl_propagate (median of %d): untilted / tilted along both axes, and the ratio" % a.repeat)
    for nx, ny, nz, P, what in ((501, 501, 20, 16, "convolution x convolution: tilted on the two-pass loop"),
                                (600, 540, 20, 16, "mixed x mixed: one-pass loop either way"),
                                (1024, 1024, 20, 16, "four-step x four-step: one-pass loop either way"),
                                (2047, 1500, 10, 4, "convolution M = 4096 x mixed: tilted on the two-pass loop")):
        flat, tilted = loop_times(nx, ny, nz, P, a.repeat)
        lines.append(f"  {nx} x {ny} x {nz} slices, {P} probes  {flat:8.3f} / {tilted:8.3f}  x {tilted / flat:5.2f}   ({what})")
    one, inner, sep = precession_times(512, 512, 16)
    lines.append("16-tilt precession run_diffraction(), 512 x 512 x 8 slices, 4 probes, 1 frame (s, set-up included / run only)")
    lines.append(f"  one precession run {one:.3f} / {inner:.3f}    16 separate single-tilt calculators {sep:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""Cost of the element maps: the reduction kernel alone for 1, 4 and 8 channels, and run_element_maps()
against run_detectors() on the same scan; written to profiles/element_signals.txt.

    python tools/element_bench.py [--out profiles/element_signals.txt] [--repeat 3] [--grid 1024] [--probes 64] [--slices 20] [--scan 8]

1. The reduction: msl_ionization_reduce repeats the tile kernel (slice_sums_kernel<IonSums>) 200 times between two events on the `probes` waves the last slice
   loop left, against the weights of one slice.  Bytes the algorithm needs per launch: 8 per pixel and image (psi, read once) and 4
   per pixel and channel (the weights, read once per chunk of images; counted once).  The share of the HBM peak is those bytes over
   the time, over 8 TB/s.  Next to it torch's device-to-device copy of the same buffer (8 bytes read and 8 written per pixel).
2. The scan: scan x scan probe positions, grid^2 pixels of 0.1 A, `slices` slices of 1 A with 40 atoms of Si and O each, probe
   batch = `probes`.  run_element_maps() with 4 channels and run_detectors() with 2 detectors alternate in one session, set up once
   each; the figure is the median.
3. Parity with the float64 definition: the figures tests/test_gpu_ionization.py prints."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EV = 100e3
HBM_PEAK = 8.0e12           # bytes / s


def source(n, nz):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(n, nz, 0.1, 1.0, n)
    rng = np.random.default_rng(5)
    pos = rng.random((40 * nz, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, len(pos))]
    return ps.Trajectory(Z, pos[None], np.zeros((1,) + pos.shape), box, 0.005), box


def channels(n):
    from pyslice_amd.ionization import Ionization
    return [Ionization((14, 8)[e % 2], 0.15 + 0.05 * e, 1.0, name=f"c{e}") for e in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "element_signals.txt"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--slices", type=int, default=20)
    ap.add_argument("--scan", type=int, default=8)
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    import torch
    import pyslice_amd as ps
    src, box = source(a.grid, a.slices)
    pp = [(box[0, 0] * (i + 0.5) / a.scan, box[1, 1] * (j + 0.5) / a.scan) for i in range(a.scan) for j in range(a.scan)]
    npix = a.grid * a.grid

    def element_calc(n):
        c = ps.MultisliceCalculator(device=0, progress=False, ionization=channels(n), probe_batch=a.probes)
        c.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=pp, sampling=0.1, slice_thickness=1.0)
        return c

    lines = ["Element maps (DESIGN.md section 4.27), written by tools/element_bench.py on an MI355X.", "",
             f"1. ion_reduce_kernel alone, {a.probes} images of {a.grid}^2, 200 launches between two events (the finishing sum of the call is in it)",
             "   bytes = 8 B x pixels x images + 4 B x pixels x channels; share of the 8 TB/s HBM peak = bytes / time / peak"]
    for n in (1, 4, 8):
        c = element_calc(n)
        res = c.run_element_maps()                              # (leaves the waves of the last probe batch in the work buffer)
        eng = c._engine
        P = eng.n_probes
        _, ms = eng.ionization_reduce(a.slices // 2, 200)
        nbytes = 8.0 * P * npix + 4.0 * n * npix
        rate = nbytes / (ms * 1e-3)
        lines.append(f"   n = {n}: {ms * 1e3:8.1f} us  {nbytes / 1e6:8.1f} MB  {rate / 1e12:5.2f} TB/s  {100.0 * rate / HBM_PEAK:5.1f} % of the HBM peak"
                     f"   (signal mean {res.signals.mean():.4e})")
        print(lines[-1], flush=True)
        if n != 4:
            eng.close()
        else:
            calc_ion, P_ion = c, P
    buf = torch.empty(P_ion * npix, dtype=torch.complex64, device="cuda")
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
    lines.append(f"   device copy of the same buffer: {ms_copy * 1e3:8.1f} us  {16.0 * P_ion * npix / (ms_copy * 1e-3) / 1e12:5.2f} TB/s read + written")
    del buf, dst

    dets = [ps.Detector("haadf", inner=60.0, outer=200.0), ps.Detector("adf", inner=30.0, outer=60.0)]
    calc_det = ps.MultisliceCalculator(device=0, progress=False, detectors=dets, probe_batch=a.probes)
    calc_det.setup(src, aperture=30.0, voltage_eV=EV, probe_positions=pp, sampling=0.1, slice_thickness=1.0)
    calc_det.run_detectors()                                    # warm-up: kernels loaded, tables made
    times = {"det": [], "ion": []}
    for _ in range(a.repeat):
        for key, run in (("det", calc_det.run_detectors), ("ion", calc_ion.run_element_maps)):
            t0 = time.perf_counter()
            run()
            times[key].append(time.perf_counter() - t0)
    det, ion = float(np.median(times["det"])), float(np.median(times["ion"]))
    lines += ["", f"2. {a.scan} x {a.scan} scan, {a.grid}^2 x {a.slices} slices, probe_batch={a.probes} (median of {a.repeat}, s; all runs)",
              f"   run_detectors(), 2 detectors (the handle's own loop)   {det:8.3f}   {' '.join(f'{t:.3f}' for t in times['det'])}",
              f"   run_element_maps(), 4 channels (two-pass loop)         {ion:8.3f}   {' '.join(f'{t:.3f}' for t in times['ion'])}",
              f"   ratio {ion / det:5.2f}   (structural expectation: the two-pass loop with the split row step, about 3.5 x the one-pass bytes)"]
    if not a.no_parity:
        lines += ["", "3. Parity with the float64 definition (tests/test_gpu_ionization.py -s)"]
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_gpu_ionization.py"), "-q", "-s", "-p",
                              "no:cacheprovider"], capture_output=True, text=True, cwd=REPO)
        lines += ["   " + m for m in re.findall(r"element maps [^\n]*", out.stdout)] + ["   pytest: " + out.stdout.strip().splitlines()[-1]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""Cost of a gradient: run_gradient() next to run_diffraction() on the same scan, in one session.

    python tools/gradient_bench.py [--out profiles/gradient.txt] [--repeat 3] [--grid 512] [--slices 100] [--scan 16] [--probe-batch 64]

The scan: scan x scan probe positions, grid^2 pixels of 0.1 A, `slices` slices of 1 A with 40 atoms of Si and O each.  The two runs
alternate, the calculators set up once each; the figure is the median.  The data of the gradient are the patterns of the same scan,
flattened a little so that the residual is not zero.  Next to the measured ratio the file states the expected ratio of the bytes the two runs move per pixel, slice and
image (the counts of section 4.31): forward 32 B (two passes, read and write), the gradient's forward 64 B (the split row step and
the copy into the stack), its backward 104 B (the step 24 B, the product 16 B, four transform passes 64 B).
The step kernel alone: msl_adjoint_step_time repeats adjoint_step_kernel 100 times between two events on the work buffer and the
stack the last batch left; the copy is torch's device-to-device copy of a buffer of the same bytes, timed the same way."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EV = 100e3


def source(n, nz):
    import pyslice_amd as ps
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(n, nz, 0.1, 1.0, n)
    rng = np.random.default_rng(5)
    pos = rng.random((40 * nz, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, len(pos))]
    return ps.Trajectory(atom_types=Z, positions=pos[None], velocities=np.zeros((1, len(pos), 3)), box_matrix=box, timestep=1.0), box


def position_leg(a, src, kw, data):
    """--positions: run_gradient() with and without Gradient(positions=True), alternating, and the chain
    alone (msl_adjoint_positions_time on the accumulator of the last run) next to the forward build of the same frame"""
    import pyslice_amd as ps
    plain = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(), probe_batch=a.probe_batch)
    plain.setup(src, **kw)
    with_pos = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(positions=True), probe_batch=a.probe_batch)
    with_pos.setup(src, **kw)
    plain.run_gradient(data)
    res = with_pos.run_gradient(data)
    times = {"plain": [], "positions": []}
    for _ in range(a.repeat):
        for name, calc in (("plain", plain), ("positions", with_pos)):
            t0 = time.perf_counter()
            res = calc.run_gradient(data)
            times[name].append(time.perf_counter() - t0)
    p, q = float(np.median(times["plain"])), float(np.median(times["positions"]))
    eng = with_pos._engine
    reps = 10
    ms_chain = eng.adjoint_positions_time(reps)
    # the forward build of the same frame by the handle's own event pair around it (msl_config.launch_timing -> counters ms_potential):
    # a handle of its own with one probe, the calculator's grid and slices
    from pyslice_amd import _native
    from pyslice_amd.potentials import loadKirkland, slice_edges
    from oracle import multislice_oracle as orc
    pos, Z = src.positions[0], src.atom_types
    xs, ys, zs = with_pos.xs, with_pos.ys, with_pos._slice_coords
    timed = _native.Engine(a.grid, a.grid, a.slices, xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], orc.wavelength(EV), orc.interaction_sigma(EV),
                           n_probes=1, launch_timing=True)
    timed.set_kirkland(loadKirkland())
    timed.set_slices(*slice_edges(zs))
    timed.build_potential(pos, Z)                               # (untimed: the form-factor tables and the allocations)
    timed.synchronize()
    timed.reset_counters()
    for _ in range(reps):
        timed.build_potential(pos, Z)
    timed.synchronize()
    ms_build = float(timed.counters()["ms_potential"]) / reps
    timed.close()
    nz, n = a.slices, len(Z)
    flops = 16.0 * n * a.grid * a.grid                           # 8 FMAs per atom and k-bin
    lines = [f"{a.scan} x {a.scan} scan, {a.grid}^2 x {a.slices} slices, {n} atoms, probe_batch={a.probe_batch} (median of {a.repeat}, s; all runs)",
             f"  run_gradient()                 {p:8.3f}   {' '.join(f'{t:.3f}' for t in times['plain'])}",
             f"  run_gradient(), positions=True {q:8.3f}   {' '.join(f'{t:.3f}' for t in times['positions'])}",
             f"  max |dL/dr| {np.abs(res.positions).max():.4e}",
             f"chain alone (Gamma -> c64, {nz} transforms, position_gradient_kernel), {reps} chains between two events",
             f"  chain {ms_chain:8.3f} ms   the kernel's 16 flops per atom and k-bin (full grid) over the WHOLE chain time: "
             f"{flops / (ms_chain * 1e-3) / 1e12:6.2f} TFLOP/s, a lower bound of the kernel's rate",
             f"  forward build of the same frame (event pair around the build, mean of {reps}) {ms_build:8.3f} ms   ratio chain / build {ms_chain / ms_build:5.2f}"]
    return lines


def probe_params_leg(a, src, kw, data):
    """--probe-params: run_gradient() with and without Gradient(probe_positions=True, aberrations=True),
    alternating, and the chain alone (msl_adjoint_probe_params_time on the work buffer of the last batch)"""
    import pyslice_amd as ps
    plain = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(), probe_batch=a.probe_batch)
    plain.setup(src, **kw)
    with_par = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(probe_positions=True, aberrations=True),
                                       probe_batch=a.probe_batch)
    with_par.setup(src, **kw)
    plain.run_gradient(data)
    res = with_par.run_gradient(data)
    times = {"plain": [], "params": []}
    for _ in range(a.repeat):
        for name, calc in (("plain", plain), ("params", with_par)):
            t0 = time.perf_counter()
            res = calc.run_gradient(data)
            times[name].append(time.perf_counter() - t0)
    p, q = float(np.median(times["plain"])), float(np.median(times["params"]))
    eng = with_par._engine
    reps = 10
    ms_chain = eng.adjoint_probe_params_time(reps)
    nz, B = a.slices, eng.n_probes
    expect = 32.0 / (168.0 * nz)                                 # one 2-D transform of the batch against the gradient's bytes per pixel
    return [f"{a.scan} x {a.scan} scan, {a.grid}^2 x {a.slices} slices, probe_batch={a.probe_batch} (median of {a.repeat}, s; all runs)",
            f"  run_gradient()                                          {p:8.3f}   {' '.join(f'{t:.3f}' for t in times['plain'])}",
            f"  run_gradient(), probe_positions=True, aberrations=True  {q:8.3f}   {' '.join(f'{t:.3f}' for t in times['params'])}",
            f"  ratio {q / p:6.4f}   expected from the bytes (32 B per pixel and image once, against 168 B per slice) {1.0 + expect:6.4f}",
            f"  max |dL/dxy| {np.abs(res.probe_position_gradient).max():.4e}  dL/dC10 {res.aberration_gradient['C10']:.4e}",
            f"chain alone (the transform of {B} images, probe_moment_kernel over the aperture's box, the sums), {reps} chains between two events",
            f"  chain {ms_chain:8.3f} ms   {32.0 * B * a.grid * a.grid / (ms_chain * 1e-3) / 1e12:6.2f} TB/s of the transform's 32 B per pixel and image"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", action="store_true", help="the position leg alone, into profiles/position_gradient.txt")
    ap.add_argument("--probe-params", action="store_true", help="the probe-parameter leg alone, into profiles/probe_gradient.txt")
    ap.add_argument("--out", default=os.path.join("profiles", "gradient.txt"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--slices", type=int, default=100)
    ap.add_argument("--scan", type=int, default=16)
    ap.add_argument("--probe-batch", type=int, default=64)
    a = ap.parse_args()
    import pyslice_amd as ps
    src, box = source(a.grid, a.slices)
    pp = [(box[0, 0] * (i + 0.5) / a.scan, box[1, 1] * (j + 0.5) / a.scan) for i in range(a.scan) for j in range(a.scan)]
    kw = dict(aperture=30.0, voltage_eV=EV, probe_positions=pp, sampling=0.1, slice_thickness=1.0)
    fwd = ps.MultisliceCalculator(device=0, progress=False, diffraction=ps.Diffraction(), probe_batch=a.probe_batch)
    fwd.setup(src, **kw)
    grad = ps.MultisliceCalculator(device=0, progress=False, gradient=ps.Gradient(), probe_batch=a.probe_batch)
    grad.setup(src, **kw)
    data = np.asarray(fwd.run_diffraction().intensity)          # warm-up, and the patterns of V
    res = grad.run_gradient(data)                               # warm-up
    # the data of the timed runs: V's own patterns give a zero residual, so they are flattened a little -- a residual of ordinary size
    data = data * 0.81 + 0.19 * data.mean(axis=(1, 2), keepdims=True)
    if a.positions:
        del grad
        text = "\n".join(position_leg(a, src, kw, data)) + "\n"
        print(text, end="")
        out = a.out if a.out != os.path.join("profiles", "gradient.txt") else os.path.join("profiles", "position_gradient.txt")
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    if a.probe_params:
        del grad
        text = "\n".join(probe_params_leg(a, src, kw, data)) + "\n"
        print(text, end="")
        out = a.out if a.out != os.path.join("profiles", "gradient.txt") else os.path.join("profiles", "probe_gradient.txt")
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    times = {"diffraction": [], "gradient": []}
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        fwd.run_diffraction()
        times["diffraction"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = grad.run_gradient(data)
        times["gradient"].append(time.perf_counter() - t0)
    d, g = float(np.median(times["diffraction"])), float(np.median(times["gradient"]))
    nz = a.slices
    expect = (64.0 * nz + 104.0 * (nz - 1) + 24.0 + 84.0) / (32.0 * nz + 16.0)
    lines = [f"{a.scan} x {a.scan} scan, {a.grid}^2 x {a.slices} slices, probe_batch={a.probe_batch} (median of {a.repeat}, s; all runs)",
             f"  run_diffraction() {d:8.3f}   {' '.join(f'{t:.3f}' for t in times['diffraction'])}",
             f"  run_gradient()    {g:8.3f}   {' '.join(f'{t:.3f}' for t in times['gradient'])}",
             f"  ratio {g / d:5.2f}   expected from the bytes per pixel and image {expect:5.2f}",
             f"  total loss {res.total:.6e}  max |dL/dV| {np.abs(res.potential).max():.4e}",
             f"  wave stack {8.0 * (nz - 1) * grad._engine.n_probes * a.grid * a.grid / 1e9:.2f} GB (pitch = ny) for {grad._engine.n_probes} probes, "
             f"accumulator {8.0 * nz * a.grid * a.grid / 1e9:.2f} GB"]
    # the step kernel alone on the work buffer of the last batch, against a device copy of the same bytes: per pixel and image the
    # step reads g and psi_s and writes g (24 B); the copy reads and writes 12 B each
    import torch
    eng = grad._engine
    P, npix, reps = eng.n_probes, a.grid * a.grid, 100
    ms = eng.adjoint_step_time(nz // 2, reps)
    eng.adjoint_reset()
    buf = torch.zeros(P * npix * 3, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(buf)
    e1.record()
    torch.cuda.synchronize()
    ms_copy = e0.elapsed_time(e1) / reps
    nbytes = 24.0 * P * npix
    r_step, r_copy = nbytes / (ms * 1e-3) / 1e12, nbytes / (ms_copy * 1e-3) / 1e12
    lines += [f"adjoint_step_kernel alone, {P} images of {a.grid}^2, slice {nz // 2}, {reps} launches between two events",
              f"  step {ms * 1e3:8.1f} us  {r_step:6.2f} TB/s read + written (24 B per pixel and image; t_s and the accumulator, 24 B per pixel, not counted)",
              f"  device copy of the same bytes {ms_copy * 1e3:8.1f} us  {r_copy:6.2f} TB/s read + written",
              f"  ratio of the rates {r_step / r_copy:5.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

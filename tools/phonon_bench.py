"""Time the potential build of phonon-mode frames: msl_build_modes (positions synthesised on the device from M modes) against
msl_build_thermal (Einstein configurations, one Philox draw per atom) and against msl_build_potentials fed the same frames from a
(B, n_atoms, 3) host array, all on the same structure and the same handle.

    python tools/phonon_bench.py [--atoms 13000] [--modes 1024] [--basis 4] [--batch 32] [--n 512] [--nz 100] [--reps 20]
                                 [--out profiles/phonon_modes.txt]

Each timing is ONE synchronous call per frame batch: the call plus msl_synchronize, wall clock.  Everything behind the positions is
the same in the three calls, so the generation of the frame batch alone is what build_modes takes beyond build_thermal (whose own
generation is one launch of n_atoms x B threads); it is printed as that difference and per (atom, mode, frame).  The last line, the
same call with M = 1, is the floor of the two launches.  The host-fed frames are the base displaced by Gaussians of 0.03 A: that
build does not care where its positions come from."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=13000, help="n_atoms (uniformly random in the box)")
    ap.add_argument("--modes", type=int, default=1024, help="M")
    ap.add_argument("--basis", type=int, default=4, help="basis atoms (more than 16: the W rows are read from global memory)")
    ap.add_argument("--batch", type=int, default=32, help="frames per call")
    ap.add_argument("--n", type=int, default=512, help="grid points per in-plane axis")
    ap.add_argument("--nz", type=int, default=100, help="slices")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    import numpy as np
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import loadKirkland, slice_edges
    from pyslice_amd.synthetic import box_for_grid

    def timed(call, eng):
        for _ in range(a.warmup):
            call()
            eng.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            eng.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    n, nz, B, M, nb, N = a.n, a.nz, a.batch, a.modes, a.basis, a.atoms
    box = box_for_grid(n, nz)
    rng = np.random.default_rng(3)
    pos = rng.random((N, 3)) * np.diag(box) * [1.0, 1.0, 0.9] + [0.0, 0.0, 0.05 * box[2, 2]]
    Z = np.array([5, 7], dtype=np.int32)[np.arange(N) % 2]
    b = (np.arange(N) % nb).astype(np.int32)
    q = (rng.random((M, 3)) - 0.5) * 2.0
    tau = rng.random(M)
    W = (rng.standard_normal((M, nb, 3)) + 1j * rng.standard_normal((M, nb, 3))) * (0.05 / np.sqrt(M))
    host = pos[None] + 0.03 * rng.standard_normal((B, N, 3))
    dx, dz = box[0, 0] / n, box[2, 2] / nz
    eng = _native.Engine(n, n, nz, dx, dx, dz, wavelength(100e3), interaction_sigma(100e3), n_probes=1, n_frames=1, frame_batch=B)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*slice_edges(np.arange(nz) * dz))
    lib = os.path.relpath(_native.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    lines = [f"# library {lib}; {a.reps} synchronous calls per line after {a.warmup} warm-up calls; ms per call of one frame "
             f"batch", f"# {n}^2 x {nz} slices, {N} atoms, {M} modes, {nb} basis atoms, frame batch {B} ({host.nbytes / 1e6:.1f} MB of "
             f"positions per host-fed call)"]
    med_p, lo, hi = timed(lambda: eng.build_potentials(host, Z), eng)
    lines.append(f"build_potentials (host array)  median {med_p:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    eng.set_structure(pos, Z, np.full(N, 0.05))
    med_t, lo, hi = timed(lambda: eng.build_thermal(11, 100, B), eng)
    lines.append(f"build_thermal    (Einstein)    median {med_t:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    eng.set_modes(b, q, tau, W, True)
    med_m, lo, hi = timed(lambda: eng.build_modes(11, 100, B), eng)
    lines.append(f"build_modes      ({M} modes)  median {med_m:.3f} ms (min {lo:.3f}, max {hi:.3f}); / build_thermal = {med_m / med_t:.3f}, "
                 f"/ build_potentials = {med_m / med_p:.3f}")
    gen = med_m - med_t
    lines.append(f"generation alone (build_modes - build_thermal): {gen:.3f} ms per batch = {gen / B * 1e3:.1f} us per frame = "
                 f"{gen * 1e9 / (float(N) * M * B):.2f} ps per (atom, mode, frame)")
    eng.set_modes(b, q[:1], tau[:1], W[:1], True)
    med_1, lo, hi = timed(lambda: eng.build_modes(11, 100, B), eng)
    lines.append(f"build_modes      (1 mode)      median {med_1:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    eng.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

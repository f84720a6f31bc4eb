"""Absorptive potential: what it costs and how close it is, written to profiles/absorptive_potential.txt.

    python tools/absorptive_bench.py [--reps 10] [--warmup 2] [--configs 64] [--out profiles/absorptive_potential.txt]

1. Timings, at the benchmark's shape (1024^2 x 200 slices, bench.py's synthetic cell) and at 512^2 x 100: the plain build of one frame
   (msl_build_potential on a handle without absorption: the code path of every earlier commit, no kernel of it was touched), the
   absorptive build of the same frame with and without Omega, and the table build (a build right after msl_set_absorption, which
   makes the tables again, minus a steady one).  One synchronous call each: the call plus msl_synchronize, wall clock, median.
2. Parity of the device build with the float64 definition: the figures tests/test_gpu_absorptive.py prints, per grid.
3. An absorptive CBED pattern next to Diffraction(split=True).elastic of a FrozenPhonons run of --configs configurations on a thin
   light specimen (BN, 256^2, 2 nm, u = 0.08 A, 100 keV, 30 mrad): recorded, not asserted -- the ensemble has its own noise,
   1 / sqrt(configs) of the thermal part, and the model its third-order error."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "absorptive_potential.txt"))
    a = ap.parse_args()
    import numpy as np
    import pyslice_amd as ps
    from pyslice_amd import _native
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import atomic_numbers_of, slice_edges
    from pyslice_amd.synthetic import synthetic_trajectory

    def timed(call, eng, before=None):
        ms = []
        for i in range(a.warmup + a.reps):
            if before is not None:
                before()
            t0 = time.perf_counter()
            call()
            eng.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    lines = ["Absorptive potential (DESIGN.md section 4.22), written by tools/absorptive_bench.py on an MI355X.", "",
             f"1. Build times, ms per synchronous call of one frame (median of {a.reps} after {a.warmup} warm-up calls; min, max)"]
    u = np.full(103, 0.08)
    for n, nz, name in ((1024, 200, "benchmark shape"), (512, 100, "512^2 x 100")):
        tr = synthetic_trajectory(n, nz, 1, seed=0)
        Z = atomic_numbers_of(tr.atom_types)
        xs, ys, zs = ps.gridFromTrajectory(tr)[:3]
        eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(100e3),
                             interaction_sigma(100e3), n_probes=1, n_frames=1)
        eng.set_kirkland(ps.loadKirkland())
        eng.set_slices(*slice_edges(zs))
        build = lambda: eng.build_potential(tr.positions[0], Z)         # noqa: E731
        plain = timed(build, eng)
        eng.set_absorption(u, True)
        full = timed(build, eng)
        with_tables = timed(build, eng, before=lambda: eng.set_absorption(u, True))
        eng.set_absorption(u, False)
        damp = timed(build, eng)
        eng.close()
        lines += [f"{name}: {len(xs)} x {len(ys)} x {len(zs)} slices, {len(Z)} atoms of {len(np.unique(Z))} species",
                  "  plain build (no absorption; the unchanged path)   %8.3f  (%.3f, %.3f)" % plain,
                  "  absorptive build, Vbar and Omega                  %8.3f  (%.3f, %.3f)   x %.2f of the plain build" % (*full, full[0] / plain[0]),
                  "  Debye-Waller damping alone (absorb = 0)           %8.3f  (%.3f, %.3f)   x %.2f" % (*damp, damp[0] / plain[0]),
                  "  absorptive build right after msl_set_absorption   %8.3f  (%.3f, %.3f)" % with_tables,
                  "  table build (that minus the steady build)         %8.3f" % (with_tables[0] - full[0])]
        print("\n".join(lines[-6:]), flush=True)

    lines += ["", "2. Parity with the float64 definition (tests/test_gpu_absorptive.py -s): fD max relative error of f D per entry; g max error",
              "   of the table over its peak; Vbar, Omega over the maximum of the float64 stack; t max |t - t_want|; bound 1e-5 max(sigma Vbar) + 2^-22"]
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_gpu_absorptive.py"), "-q", "-s", "-p",
                          "no:cacheprovider", "-k", "tables_and_transmission or run_end_to_end or thickness"], capture_output=True, text=True, cwd=REPO)
    lines += ["   " + m for m in re.findall(r"absorptive [^\n]*", out.stdout)] + ["   pytest: " + out.stdout.strip().splitlines()[-1]]

    lines += ["", f"3. CBED: absorptive pattern next to the elastic part of {a.configs} frozen-phonon configurations (recorded, not asserted)"]
    tr = synthetic_trajectory(256, 40, 1, seed=5)
    pp = [(12.8, 12.8), (11.1, 13.9)]
    fp = ps.FrozenPhonons.from_trajectory(tr, 0.08, a.configs, seed=1)

    def pattern(source, diffraction):
        calc = ps.MultisliceCalculator(device=0, progress=False, diffraction=diffraction)
        calc.setup(source, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
        t0 = time.perf_counter()
        res = calc.run_diffraction()
        return res, time.perf_counter() - t0
    ens, t_ens = pattern(fp, Diffraction(split=True))
    elastic = np.asarray(ens.elastic)
    rel = lambda x, y: float(np.linalg.norm((x - y).ravel()) / np.linalg.norm(y.ravel()))      # noqa: E731
    rows = [("absorptive (Vbar and Omega)", fp.absorptive()), ("Debye-Waller damping alone", fp.absorptive(absorption=False)),
            ("static potential (no vibration)", tr)]
    lines.append(f"   256 x 256 x {len(ps.gridFromTrajectory(tr)[2])} slices of 0.5 A, {fp.n_atoms} atoms (B, N), u = 0.08 A, 30 mrad, 100 keV, 2 probes; ensemble run {t_ens:.3f} s; "
                 f"elastic part {elastic.sum() / np.asarray(ens.intensity).sum():.4f} of the ensemble's total intensity")
    for name, src in rows:
        res, t = pattern(src, Diffraction())
        I = np.asarray(res.intensity)
        lines.append(f"   {name:34s} rel-L2 to the elastic part {rel(I, elastic):.3e}   total / elastic total {I.sum() / elastic.sum():.5f}   run {t:.3f} s")
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

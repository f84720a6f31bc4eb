"""Specimen tilt on the MI355X: the propagator tables msl_set_tilt writes on the device (csrc/propagator.h) against the float64
definition (pyslice_amd/tilt.py), on one grid per table form, with nz = 3 and 1-2 probes.

Bounds.  The tilt only changes the values in tables the slice loop reads anyway, so a tilted run may carry the fp32 error of the
untilted run of the same case and no more: every comparison allows TWICE the error of the untilted run against float64, measured
in the same test (rel-L2 over the exit waves, the metric of tests/test_gpu_parity.py).  The untilted tables written by the device
differ from the host's by at most one float rounding per entry (2^-24 relative), per axis and slice: max|d psi| / max|psi| <=
2 nz 2^-24.  Runs that make the same launches on the same tables are bit-identical (no atomics anywhere on the path).

Kinds per grid, from plan_axis_kind (a register kernel along an axis needs the OTHER length to be a multiple of 16):
    256 x 96     four-step R = 16  x  convolution M = 256
    512 x 200    convolution M = 1024  x  convolution M = 1024        (200 lines are no multiple of 16: 512 is no AX_TWO here)
    600 x 540    mixed 25 * 24  x  mixed 27 * 20, both over an AX_CONV2K base (filters of M = 2048 written, the passes read the plain tables)
    1024 x 1000  convolution M = 2048  x  mixed 2 * 25 * 20                (1000 lines: 1024 is no four-step axis here)
    1100 x 2048  the two-pass loop on the plain tables (1100 lines: 2048 is no AX_WAVE2K here; the M = 4096 filter is written, not read)
and, beyond the grids the feature was specified with:
    512 x 512    AX_TWO x AX_TWO (split-order tables)
    1024 x 1120  four-step R = 32  x  mixed 2 * 28 * 20
    1104 x 2048  AX_CONV4K (even-odd filter of M = 4096)  x  AX_WAVE2K

The convolution passes (AX_CONV, AX_CONV2K, AX_CONV4K) keep half of their filter and mirror the other half, and the 2048-point wave
kernel reads its Fresnel factors the same way; a tilted axis has no even table (one axis tilted at a time on tilted tables: rel-L2 1.0
to 1.1 against the rolled wave along those axes, 3e-7 along every other).  msl_set_tilt therefore runs a tilt along such an axis on the
two-pass loop, and comes back to the one-pass loop at a zero tangent: 256 x 96 (y), 512 x 200, 1024 x 1000 (x) and 1104 x 2048 below.
"""
import functools

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

EV, MRAD = 100e3, 30.0
NZ, DZ, SAMPLING = 3, 2.0, 0.1
GRIDS = [(256, 96, 2), (512, 200, 2), (600, 540, 2), (1024, 1000, 2), (1100, 2048, 1), (512, 512, 2), (1024, 1120, 2), (1104, 2048, 1)]
IDS = [f"{nx}x{ny}" for nx, ny, _ in GRIDS]


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def max_rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _trajectory(nx, ny, seed=0):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(nx, NZ, 1, ny=ny, slice_thickness=DZ, density=0.03, seed=seed + nx + 7 * ny)


def _grid(tr):
    from oracle import multislice_oracle as orc
    xs, ys, zs, *_ = orc.grid_from_box(tr.box_matrix, sampling=SAMPLING, slice_thickness=DZ)
    return np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.asarray(zs, dtype=np.float64)


def _positions(xs, ys, P):
    lx, ly = len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])
    return np.asarray([(0.31 * lx, 0.62 * ly), (0.77 * lx, 0.18 * ly)][:P], dtype=np.float64)


def _engine(xs, ys, zs, P, **kw):
    from pyslice_amd import _native
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.potentials import loadKirkland, slice_edges
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], wavelength(EV), interaction_sigma(EV),
                         n_probes=P, **kw)
    eng.set_kirkland(loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.set_probes(MRAD, _positions(xs, ys, P))
    return eng


def _exit(eng):
    eng.propagate()
    return eng.exit_waves().copy()


# ------------------------------------------------------------------ 1 + 3. vacuum: whole-pixel shifts, and the untilted tables
@functools.lru_cache(maxsize=None)
def vacuum_case(nx, ny, P):
    """every vacuum run of one grid, made once: two handles that never see msl_set_tilt, then on the first (0, 0), the whole-pixel
    tilt (+3 px in x, -2 px in y per slice), and (0, 0) again; and the float64 untilted exit waves from the device's own probes"""
    from pyslice_amd.multislice import wavelength
    from pyslice_amd.tilt import propagate_tilted
    xs, ys, zs = _grid(_trajectory(nx, ny))
    assert (len(xs), len(ys), len(zs)) == (nx, ny, NZ)
    dx, dy, dz = xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]
    V0 = np.zeros((NZ, nx, ny), dtype=np.float32)
    out = {}
    a, b = _engine(xs, ys, zs, P), _engine(xs, ys, zs, P)
    try:
        for eng in (a, b):
            eng.upload_potential(V0)
        out["never"], out["never2"] = _exit(a), _exit(b)
        out["tilt_before"] = a.get_tilt()
        psi0 = a.probes().astype(np.complex128)
        a.set_tilt(0.0, 0.0)
        out["zero"] = _exit(a)
        tan = (3 * dx / dz, -2 * dy / dz)
        a.set_tilt(*tan)
        out["tilt_after"], out["tan"] = a.get_tilt(), tan
        out["tilted"] = _exit(a)
        a.set_tilt(0.0, 0.0)
        out["zero_again"] = _exit(a)
    finally:
        a.close()
        b.close()
    out["flat64"] = propagate_tilted(psi0, np.ones((NZ, nx, ny)), dx, dy, wavelength(EV), dz)
    return out


@pytest.mark.parametrize("nx,ny,P", GRIDS, ids=IDS)
def test_vacuum_shift_through_the_library(nx, ny, P):
    c = vacuum_case(nx, ny, P)
    assert c["tilt_before"] == (0.0, 0.0) and c["tilt_after"] == c["tan"]
    want = np.roll(c["flat64"], (3 * (NZ - 1), -2 * (NZ - 1)), axis=(1, 2))
    e0, e1 = rel_l2(c["never"], c["flat64"]), rel_l2(c["tilted"], want)
    print(f"tilt vacuum {nx} x {ny}: untilted fp32 rel-L2 {e0:.3e} (max {max_rel(c['never'], c['flat64']):.3e}), "
          f"tilted {e1:.3e} (max {max_rel(c['tilted'], want):.3e}), bound {2 * e0:.3e}")
    assert e0 < 1e-5                                                     # (the untilted run is a sound yardstick: fp32 rounding only)
    assert e1 <= 2 * e0
    assert rel_l2(c["tilted"], c["flat64"]) > 0.3                         # (the shift of 6 and -4 pixels is of the size of the probe: no no-op)


@pytest.mark.parametrize("nx,ny,P", GRIDS, ids=IDS)
def test_untilted_outputs_unchanged(nx, ny, P):
    c = vacuum_case(nx, ny, P)
    assert np.array_equal(c["never"], c["never2"])                        # never tilted: bit for bit the run of old
    d = max_rel(c["zero"], c["never"])
    print(f"tilt zero {nx} x {ny}: max|d psi| / max|psi| {d:.3e}, bound {2 * NZ * 2.0 ** -24:.3e}")
    assert d <= 2 * NZ * 2.0 ** -24
    assert np.array_equal(c["zero"], c["zero_again"])                     # (0, 0) after a tilt restores the untilted tables


# ------------------------------------------------------------------ 2. with atoms, a fractional-pixel tilt
@pytest.mark.parametrize("nx,ny,P", GRIDS, ids=IDS)
def test_tilted_run_with_atoms_matches_the_float64_definition(nx, ny, P):
    from oracle import multislice_oracle as orc
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.tilt import Tilt, propagate_tilted
    tr = _trajectory(nx, ny, seed=1)
    xs, ys, zs = _grid(tr)
    tilt = Tilt(118.0, -71.0)                                            # 2.37 px in x, -1.42 px in y per slice
    eng = _engine(xs, ys, zs, P, keep_potential=True)
    try:
        eng.build_potential(tr.positions[0], np.asarray(tr.atom_types, dtype=np.int32))
        V = eng.potential().astype(np.float64)                          # (nz, nx, ny): both float64 runs start from the device's V
        psi0 = eng.probes().astype(np.complex128)
        flat = _exit(eng)
        eng.set_tilt(*tilt.tangents)
        tilted = _exit(eng)
    finally:
        eng.close()
    assert np.ptp(V) > 1.0                                               # (there are atoms)
    want0 = orc.propagate(psi0, np.moveaxis(V, 0, 2), xs, ys, zs, EV, workers=min(16, orc.usable_cores()))
    want = propagate_tilted(psi0, np.exp(1j * interaction_sigma(EV) * V), xs[1] - xs[0], ys[1] - ys[0], wavelength(EV), zs[1] - zs[0], tilt)
    e0, e1 = rel_l2(flat, want0), rel_l2(tilted, want)
    print(f"tilt atoms {nx} x {ny}: untilted vs oracle rel-L2 {e0:.3e}, tilted vs definition {e1:.3e}, bound {2 * e0:.3e}")
    assert e0 < 1e-4                                                     # the contract of tests/test_gpu_parity.py
    assert e1 <= 2 * e0
    assert rel_l2(want, want0) > 0.1                                     # (the tilt matters in this case)


# ------------------------------------------------------------------ 4. the layer tap under tilt (the conjugate tables), through the calculator
def test_layer_tap_under_tilt():
    import pyslice_amd as ps
    from oracle import multislice_oracle as orc
    from pyslice_amd.multislice import interaction_sigma, wavelength
    from pyslice_amd.tilt import Tilt, propagate_tilted
    nx, ny, P = 256, 96, 2
    tr = _trajectory(nx, ny, seed=2)
    xs, ys, zs = _grid(tr)
    pp = [tuple(p) for p in _positions(xs, ys, P)]
    tilt = Tilt(118.0, -71.0)
    got = {}
    for name, t in (("flat", None), ("tilted", tilt)):
        calc = ps.MultisliceCalculator(progress=False, dtype="complex64", layers=[1], tilt=t)
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
        assert (calc.nx, calc.ny, calc.nz) == (nx, ny, NZ)
        wf = calc.run()
        assert list(wf.layer) == [1, NZ - 1]
        got[name] = npy(wf.wavefunction_data)[:, 0]                      # (P, nx, ny, L)
    V = orc.potential(xs, ys, zs, tr.positions[0], tr.atom_types)
    psi0 = orc.batched_probes(orc.probe_array(xs, ys, MRAD, EV), xs, ys, pp)
    trans = np.exp(1j * interaction_sigma(EV) * np.moveaxis(V, 2, 0))
    for name, t in (("flat", None), ("tilted", tilt)):
        ex, taps = propagate_tilted(psi0, trans, xs[1] - xs[0], ys[1] - ys[0], wavelength(EV), zs[1] - zs[0], t, layers=[1])
        got[name + "64"] = np.stack([orc.diffraction(taps[1]), orc.diffraction(ex)], axis=-1)
    for li, k in enumerate((1, NZ - 1)):
        e0 = rel_l2(got["flat"][..., li], got["flat64"][..., li])
        e1 = rel_l2(got["tilted"][..., li], got["tilted64"][..., li])
        print(f"tilt layer {k} 256 x 96: untilted rel-L2 {e0:.3e}, tilted {e1:.3e}, bound {2 * e0:.3e}")
        assert e0 < 1e-4 and e1 <= 2 * e0, k
        assert rel_l2(got["tilted64"][..., li], got["flat64"][..., li]) > 0.1, k


# ------------------------------------------------------------------ 5. precession
def test_precession_is_the_mean_of_its_tilts():
    import pyslice_amd as ps
    nx, ny, P = 256, 96, 2
    tr = _trajectory(nx, ny, seed=3)
    xs, ys, zs = _grid(tr)
    pp = [tuple(p) for p in _positions(xs, ys, P)]
    pre = ps.Precession(10.0, 4)

    def run(**kw):
        calc = ps.MultisliceCalculator(progress=False, diffraction=ps.Diffraction(), **kw)
        calc.setup(tr, aperture=MRAD, voltage_eV=EV, probe_positions=pp, slice_thickness=DZ, sampling=SAMPLING)
        return calc.run_diffraction()
    res = run(precession=pre)
    assert res.tilts == pre.tilts() and res.intensity.shape == (P, nx, ny)
    mean = np.zeros_like(res.intensity)
    for t in pre.tilts():
        single = run(tilt=t)
        assert single.tilts is None
        mean += single.intensity
    mean /= 4
    flat = run().intensity
    d, moved = max_rel(res.intensity, mean), max_rel(flat, mean)
    print(f"tilt precession 256 x 96: against the mean of the single-tilt runs {d:.3e}, untilted pattern against it {moved:.3e}")
    assert d <= 1e-12
    assert moved > 1e-6                                                  # no no-op: well above what the float rounding of a table could move
    assert abs(res.intensity.sum() / flat.sum() - 1.0) < 1e-4            # a tilt is unitary: the same electrons


# ------------------------------------------------------------------ 6. stream ordering
def test_two_tilts_back_to_back_without_a_wait():
    """set_tilt, slice loop, set_tilt, slice loop, all queued before anything is waited for: the second tilt's tables (and the float64
    scratch of its convolution sums) are written behind the first tilt's passes.  600 x 540: plain tables read by the passes, and
    the filters of the AX_CONV2K bases written through the shared scratch in between"""
    nx, ny, P = 600, 540, 2
    tr = _trajectory(nx, ny, seed=4)
    xs, ys, zs = _grid(tr)
    t1, t2 = (0.118, -0.071), (-0.05, 0.16)
    eng = _engine(xs, ys, zs, P, n_frames=2)
    try:
        eng.build_potential(tr.positions[0], np.asarray(tr.atom_types, dtype=np.int32))
        eng.set_tilt(*t1)
        eng.propagate_frame(0)
        eng.set_tilt(*t2)
        eng.propagate_frame(1)
        both = eng.wavefunction().copy()                                 # (P, 2, nx, ny): the first wait
        singles = []
        for t in (t1, t2):
            eng.set_tilt(*t)
            eng.synchronize()
            eng.propagate_frame(0)
            eng.synchronize()
            singles.append(eng.wavefunction()[:, 0].copy())
    finally:
        eng.close()
    assert np.array_equal(both[:, 0], singles[0]) and np.array_equal(both[:, 1], singles[1])
    assert rel_l2(singles[0], singles[1]) > 0.1


def test_loop_switch_carries_a_built_potential_both_ways():
    """256 x 96, potential built while the one-pass loop is on (every second slice lives transposed), then a tilt along y (convolution:
    the two-pass loop takes over and needs those slices in natural order), (0, 0) again, the tilt again: the transposes of the switch are
    exact, so each pair of runs is bit-identical.  A stack built under the tilt comes from another inverse transform of the potential
    build (PI_LINES): the same wave to twice the 1e-4 of the parity contract (tests/test_gpu_parity.py)"""
    nx, ny, P = 256, 96, 2
    tr = _trajectory(nx, ny, seed=5)
    xs, ys, zs = _grid(tr)
    Z = np.asarray(tr.atom_types, dtype=np.int32)
    eng = _engine(xs, ys, zs, P)
    try:
        eng.build_potential(tr.positions[0], Z)
        eng.set_tilt(0.0, 0.0)
        flat_a = _exit(eng)
        eng.set_tilt(0.05, -0.12)
        tilted_a = _exit(eng)                                            # stack carried over to the two-pass loop
        eng.set_tilt(0.0, 0.0)
        flat_b = _exit(eng)                                              # carried back to the one-pass loop
        eng.set_tilt(0.05, -0.12)
        tilted_b = _exit(eng)
        eng.build_potential(tr.positions[0], Z)
        tilted_c = _exit(eng)                                            # stack built under the tilt
        eng.set_tilt(0.05, 0.0)
        x_only = _exit(eng)                                              # a tilt along the four-step axis alone: the one-pass loop
    finally:
        eng.close()
    assert np.array_equal(flat_a, flat_b) and np.array_equal(tilted_a, tilted_b)
    assert rel_l2(tilted_c, tilted_a) < 2e-4
    assert rel_l2(tilted_a, flat_a) > 0.1 and rel_l2(x_only, flat_a) > 0.05 and rel_l2(x_only, tilted_a) > 0.05


def test_set_tilt_refuses_non_finite_tangents():
    xs, ys, zs = _grid(_trajectory(256, 256))
    eng = _engine(xs, ys, zs, 1)
    try:
        eng.set_tilt(0.1, -0.2)
        for bad in ((float("nan"), 0.0), (0.0, float("inf"))):
            with pytest.raises(ValueError, match="msl_set_tilt"):
                eng.set_tilt(*bad)
        assert eng.get_tilt() == (0.1, -0.2)                             # a refused call leaves the tilt as it was
    finally:
        eng.close()

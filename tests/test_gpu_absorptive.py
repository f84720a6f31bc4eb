"""Absorptive potential on the MI355X: the tables the device builds, the complex transmission functions and the runs through them
against the NumPy definition (pyslice_amd/absorptive.py) carried through the float64 oracle.

Cells: 40 atoms per slice of Si and O (u = 0.078 / 0.09 A), uniformly random, 0.1 A pixels, 1 A slices, 100 kV.  The grids take every
2-D transform family of the potential build and both loop forms: 64 x 48 and 96 x 80 (convolution kernels), 101 x 97 (odd: generic
lines), 135 x 150 (mixed radix), 256 x 256 (four-step on both axes, half rows), 512 x 256 (2 R^2 next to four-step).

Bounds.  Tables: f D one float32 rounding of the float64 value, 2^-23 relative with the float32 Kirkland sum under it.  Transmission:
the project's potential contract carried to the complex potential, max |t - t_want| <= 1e-5 max(sigma Vbar) + 2^-22.  Runs: the
wavefunction contract, rel-L2 <= 1e-4."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from oracle import multislice_oracle as orc

pytestmark = pytest.mark.gpu

EV = 100e3
U = {14: 0.078, 8: 0.09}
GRIDS = [(64, 48, 3), (96, 80, 4), (101, 97, 3), (135, 150, 3), (256, 256, 3), (512, 256, 3)]
PP = [(3.05, 4.4), (1.7, 1.25)]


def npy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


@functools.lru_cache(maxsize=None)
def source(nx, ny, nz, absorption=True):
    from pyslice_amd.absorptive import AbsorptivePotential
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(nx, nz, 0.1, 1.0, ny)
    rng = np.random.default_rng(nx + ny + nz)
    n = 40 * nz
    pos = rng.random((n, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, n)]
    ap = AbsorptivePotential(Z, pos, box, U, absorption=absorption)
    ap.base_positions.setflags(write=False)
    return ap


def stack_from_tables(xs, ys, zs, pos, Z, tables):
    """(nz, nx, ny) float64: the oracle's potential (multislice_oracle.potential, slice axis 2) with tables[Z] (nx, ny) in the place of
    f_Z(q^2) -- its slice bins, its structure-factor sum, its inverse transform and 1 / (dx^2 dy^2), restated with the table an argument"""
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    lo, hi = orc.slice_edges(zs)
    kxs, kys = np.fft.fftfreq(len(xs), d=dx), np.fft.fftfreq(len(ys), d=dy)
    recip = np.zeros((len(zs), len(xs), len(ys)), dtype=np.complex128)
    for z in np.unique(Z):
        sel = pos[Z == z]
        for s in range(len(zs)):
            m = (sel[:, 2] >= lo[s]) & (sel[:, 2] < hi[s])
            if m.any():
                recip[s] += (np.exp(-2j * np.pi * np.outer(kxs, sel[m, 0])) @ np.exp(-2j * np.pi * np.outer(sel[m, 1], kys))) * tables[int(z)]
    return np.fft.ifft2(recip, axes=(1, 2)).real / (dx ** 2 * dy ** 2)


@functools.lru_cache(maxsize=None)
def want(nx, ny, nz, eV=EV):
    """float64: the tables (f D, g) per species, Vbar and Omega (nz, nx, ny) from the oracle's potential with those tables in the
    place of its form factor (stack_from_tables, pinned to the oracle with its own tables), sigma, and the grid axes; computed once
    per grid, read-only"""
    from pyslice_amd.absorptive import absorptive_tables
    import pyslice_amd
    ap = source(nx, ny, nz)
    xs, ys, zs = pyslice_amd.gridFromTrajectory(ap, 0.1, 1.0)[:3]
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    q2 = np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2
    tables = {Z: absorptive_tables(orc.form_factor(q2, Z), q2, U[Z], dx, dy) for Z in (8, 14)}
    pos, Zs = ap.base_positions, np.asarray(ap.atom_types)
    plain = stack_from_tables(xs, ys, zs, pos, Zs, {Z: orc.form_factor(q2, Z) for Z in (8, 14)})
    assert np.abs(plain - np.moveaxis(orc.potential(xs, ys, zs, pos, Zs), 2, 0)).max() <= 1e-12 * np.abs(plain).max()
    stacks = [stack_from_tables(xs, ys, zs, pos, Zs, {Z: tables[Z][k] for Z in (8, 14)}) for k in (0, 1)]
    out = dict(fD=np.stack([tables[8][0], tables[14][0]]), g=np.stack([tables[8][1], tables[14][1]]), Vbar=stacks[0], Om=stacks[1],
               sigma=orc.interaction_sigma(eV), xs=xs, ys=ys, zs=zs)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def make_engine(ps, ap, absorb=True, set_abs=True, eV=EV, **kw):
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    xs, ys, zs = ps.gridFromTrajectory(ap, 0.1, 1.0)[:3]
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], orc.wavelength(eV),
                         orc.interaction_sigma(eV), n_probes=len(PP), **kw)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    if set_abs:
        eng.set_absorption(ap.u_by_Z, absorb)
    return eng


def t_bound(w):
    return 1e-5 * np.abs(w["sigma"] * w["Vbar"]).max() + 2.0 ** -22


@pytest.mark.parametrize("grid", GRIDS)
def test_tables_and_transmission(ps, grid):
    """MSL_BUF_FORMFACTOR is f D to 2^-23 relative per entry; g is held through the potential it makes: Omega and Vbar to 1e-5 of their
    maxima, and t = exp(i sigma Vbar - sigma^2 Omega) to the bound of the module"""
    from pyslice_amd.absorptive import absorptive_transmission
    ap, w = source(*grid), want(*grid)
    eng = make_engine(ps, ap)
    eng.build_potential(ap.base_positions, ap.atom_types)
    fD, g = eng.form_factors(2).astype(np.float64), eng.form_factors_abs(2).astype(np.float64)
    e_fd = np.abs(fD / w["fD"] - 1.0).max()
    e_g = np.abs(g - w["g"]).max() / np.abs(w["g"]).max()
    Vbar, Om, t = eng.potential().astype(np.float64), eng.absorption().astype(np.float64), eng.transmission().astype(np.complex128)
    e_v = np.abs(Vbar - w["Vbar"]).max() / np.abs(w["Vbar"]).max()
    e_o = np.abs(Om - w["Om"]).max() / np.abs(w["Om"]).max()
    e_t = np.abs(t - absorptive_transmission(w["Vbar"], w["Om"], w["sigma"])).max()
    print(f"absorptive {grid}: fD {e_fd:.2e} g {e_g:.2e} Vbar {e_v:.2e} Omega {e_o:.2e} t {e_t:.2e} bound {t_bound(w):.2e} "
          f"max sigma Vbar {np.abs(w['sigma'] * w['Vbar']).max():.2f} min |t| {np.abs(t).min():.4f}")
    assert e_fd <= 2.0 ** -23
    assert e_g <= 1e-5          # the potential contract on the table itself: Omega is linear in g, entry by entry of unit weight
    assert e_v <= 1e-5 and e_o <= 1e-5
    assert e_t <= t_bound(w)
    assert np.abs(t).min() < 0.999          # (no upper bound on |t|: the band-limited Omega rings slightly below zero between the atoms)


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[2], GRIDS[4]])
def test_damping_alone_has_unit_modulus(ps, grid):
    ap, w = source(*grid), want(*grid)
    eng = make_engine(ps, ap, absorb=False)
    eng.build_potential(ap.base_positions, ap.atom_types)
    t = eng.transmission().astype(np.complex128)
    assert np.abs(np.abs(t) - 1.0).max() <= 2.0 ** -22
    assert np.abs(t - np.exp(1j * w["sigma"] * w["Vbar"])).max() <= t_bound(w)
    assert eng.buffer_bytes(14) == 0 and eng.buffer_bytes(13) == 0


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[4], GRIDS[5]])
def test_clearing_restores_the_plain_build_bit_for_bit(ps, grid):
    ap = source(*grid)
    eng = make_engine(ps, ap)
    eng.build_potential(ap.base_positions, ap.atom_types)
    eng.set_absorption(None)
    eng.build_potential(ap.base_positions, ap.atom_types)
    fresh = make_engine(ps, ap, set_abs=False)
    fresh.build_potential(ap.base_positions, ap.atom_types)
    assert eng.transmission().tobytes() == fresh.transmission().tobytes()
    assert eng.form_factors(2).tobytes() == fresh.form_factors(2).tobytes()
    assert eng.buffer_bytes(2) == 0 and eng.buffer_bytes(14) == 0


def float64_exit(w, nx, ny, nz, absorb=True):
    """the float64 slice loop through the complex transmission: the oracle's propagate takes V = Vbar + i sigma Omega"""
    V = np.moveaxis(w["Vbar"] + (1j * w["sigma"] * w["Om"] if absorb else 0.0), 0, 2)
    probes = orc.batched_probes(orc.probe_array(w["xs"], w["ys"], 30.0, EV), w["xs"], w["ys"], PP)
    return probes, orc.propagate(probes, V, w["xs"], w["ys"], w["zs"], EV)


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[4]])
@pytest.mark.parametrize("absorption", [True, False])
def test_run_end_to_end(ps, grid, absorption):
    ap, w = source(*grid, absorption), want(*grid)
    calc = ps.MultisliceCalculator(device=0, progress=False)
    calc.setup(ap, aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=0.1, slice_thickness=1.0)
    got = npy(calc.run().wavefunction_data)[:, 0, :, :, 0]
    probes, ex = float64_exit(w, *grid, absorb=absorption)
    ref = orc.diffraction(ex)
    assert rel_l2(got, ref) <= 1e-4
    n0, n_got, n_ref = (np.abs(probes) ** 2).sum(), (np.abs(got) ** 2).sum() / (grid[0] * grid[1]), (np.abs(ex) ** 2).sum()
    print(f"absorptive run {grid} absorption={absorption}: rel-L2 {rel_l2(got, ref):.2e}, norm in {n0:.6f} out {n_got:.6f} float64 {n_ref:.6f}")
    assert abs(n_got / n_ref - 1.0) <= 1e-4
    if absorption:
        assert n_ref < n0 * (1.0 - 1e-4) and n_got < n0      # (the float64 loss is far above the 1e-5 to which fp32 conserves)
    else:
        assert abs(n_got / n0 - 1.0) <= 1e-5


def test_tilted_thickness_series_and_images_see_the_complex_transmission(ps):
    """96 x 80 x 4: run_diffraction() with tilt= and thickness=[1, 3] -- the tilted propagator tables and the layer taps behind a
    transmission with |t| != 1 -- and run_images(), each entry against the float64 loop (tilt.propagate_tilted) through the complex
    transmission of the definition, stopped after slices 1 and 3.  Intensities: twice the wavefunction contract, 2e-4 rel-L2."""
    from pyslice_amd.absorptive import absorptive_transmission
    from pyslice_amd.diffraction_data import Diffraction
    from pyslice_amd.imaging import Imaging
    from pyslice_amd.tilt import Tilt, propagate_tilted
    grid = GRIDS[1]
    ap, w = source(*grid), want(*grid)
    xs, ys, zs = w["xs"], w["ys"], w["zs"]
    geom = (xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0])
    t_abs = absorptive_transmission(w["Vbar"], w["Om"], w["sigma"])
    t_damp = np.exp(1j * w["sigma"] * w["Vbar"])
    probes = orc.batched_probes(orc.probe_array(xs, ys, 30.0, EV), xs, ys, PP)
    tilt = Tilt(118.0, -71.0)
    calc = ps.MultisliceCalculator(device=0, progress=False, diffraction=Diffraction(), tilt=tilt, thickness=[1, 3])
    calc.setup(ap, aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=0.1, slice_thickness=1.0)
    res = calc.run_diffraction()
    pat = np.asarray(res.intensity)
    assert list(res.layer) == [1, 3] and pat.shape == (len(PP), grid[0], grid[1], 2)
    ex, taps = propagate_tilted(probes, t_abs, *geom, tilt, layers=[1])
    flat = propagate_tilted(probes, t_abs, *geom, None)
    damp, damp_taps = propagate_tilted(probes, t_damp, *geom, tilt, layers=[1])
    for li, (wave, unabsorbed) in enumerate(((taps[1], damp_taps[1]), (ex, damp))):
        ref = np.abs(orc.diffraction(wave)) ** 2
        err = rel_l2(pat[..., li], ref)
        print(f"absorptive tilted thickness entry {li}: rel-L2 {err:.2e}")
        assert err <= 2e-4, li
        assert rel_l2(ref, np.abs(orc.diffraction(unabsorbed)) ** 2) > 1e-3, li          # (the absorption matters in this entry)
    assert rel_l2(np.abs(orc.diffraction(ex)) ** 2, np.abs(orc.diffraction(flat)) ** 2) > 0.1           # (and so does the tilt)
    calc = ps.MultisliceCalculator(device=0, progress=False, imaging=Imaging())
    calc.setup(ap, aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=0.1, slice_thickness=1.0)
    img = np.asarray(calc.run_images().intensity)[:, 0, 0]
    assert rel_l2(img, np.abs(flat) ** 2) <= 2e-4
    assert img.sum() < 0.999 * (np.abs(propagate_tilted(probes, t_damp, *geom, None)) ** 2).sum()


def test_frame_batch_slots_and_unaligned_stacks(ps):
    """101 x 97 x 3 at frame_batch = 2: a stack is 29 391 pixels, so the second slot of every buffer starts off a 16-byte boundary --
    the pixel-by-pixel form of the epilogue, the slot offsets of the real stores, and msl_set_beam over every slot"""
    from pyslice_amd.absorptive import absorptive_transmission
    grid = GRIDS[2]
    ap, w = source(*grid), want(*grid)
    assert (grid[0] * grid[1] * grid[2] * 4) % 16 != 0
    eng = make_engine(ps, ap, frame_batch=2, n_frames=2)
    assert eng.frame_batch == 2
    eng.build_potentials(np.stack([ap.base_positions, ap.base_positions]), ap.atom_types)
    for sigma in (w["sigma"], orc.interaction_sigma(200e3)):
        t_want = absorptive_transmission(w["Vbar"], w["Om"], sigma)
        for slot in (1, 0):
            eng.select_batch_slot(slot)
            assert np.abs(eng.transmission().astype(np.complex128) - t_want).max() <= t_bound(w), (sigma, slot)
            assert np.abs(eng.absorption().astype(np.float64) - w["Om"]).max() <= 1e-5 * np.abs(w["Om"]).max(), slot
        eng.set_beam(orc.wavelength(200e3), orc.interaction_sigma(200e3), 1.0)


def test_toggling_absorption_forgets_the_built_stacks(ps):
    """msl_set_absorption on a handle with a build: the stacks no longer say what the next msl_set_beam should make, so the potential
    counts as not built until the next build"""
    ap = source(*GRIDS[0])
    eng = make_engine(ps, ap)
    eng.build_potential(ap.base_positions, ap.atom_types)
    assert eng.buffer_bytes(14) > 0
    eng.set_absorption(ap.u_by_Z, False)
    assert eng.buffer_bytes(14) == 0 and eng.buffer_bytes(2) == 0
    eng.set_beam(orc.wavelength(200e3), orc.interaction_sigma(200e3), 1.0)       # (nothing to recompute: no error)
    eng.build_potential(ap.base_positions, ap.atom_types)
    assert np.abs(np.abs(eng.transmission()) - 1.0).max() <= 2.0 ** -22


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[4]])
def test_set_beam_recomputes_t_from_the_two_stacks(ps, grid):
    ap = source(*grid)
    eng = make_engine(ps, ap, keep_potential=True)
    eng.build_potential(ap.base_positions, ap.atom_types)
    eng.set_beam(orc.wavelength(200e3), orc.interaction_sigma(200e3), 1.0)
    fresh = make_engine(ps, ap, eV=200e3, keep_potential=True)
    fresh.build_potential(ap.base_positions, ap.atom_types)
    assert eng.transmission().tobytes() == fresh.transmission().tobytes()
    assert eng.absorption().tobytes() == fresh.absorption().tobytes()


def test_thermal_builds_are_refused_while_absorption_is_set(ps):
    from pyslice_amd import _native
    ap = source(*GRIDS[0])
    eng = make_engine(ps, ap)
    eng.set_structure(ap.base_positions, ap.atom_types, ap.sigma, 2)
    assert eng._lib.msl_build_thermal(eng._h, 1, 0, 1) == _native.MSL_ERR_STATE
    assert eng._lib.msl_build_modes(eng._h, 1, 0, 1) == _native.MSL_ERR_STATE
    eng.set_absorption(None)
    eng.build_thermal(1, 0, 1)

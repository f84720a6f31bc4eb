"""TDS detector signal of the absorptive potential on the MI355X: the detector-restricted tables and the weight stack the device
builds, the TDS slice loop and its reduction, and run_detectors(tds=True), against the float64 definition (pyslice_amd/tds.py).

Cells as in test_gpu_absorptive.py (its sources and float64 stacks are shared): 40 atoms per slice of Si and O, u = 0.078 / 0.09 A,
0.1 A pixels, 1 A slices, 100 kV; 3 probes, a count that is no multiple of any probe chunk.  Grids: 256 x 64 and 64 x 256 (the fast
row kernel on ny = 256), 96 x 80 x 4 (generic lines), 101 x 97 (odd: the pitch tail of the 16-byte loads).

Bounds.  g_det and Omega_det: the bounds test_gpu_absorptive.py puts on g and Omega, 1e-5 of their maxima.  w = 1 - exp(-2 sigma^2
Omega_det): |dw| <= 2 sigma^2 |dOmega| (the slope of 1 - exp(-x) is at most 1 where Omega >= 0, and e^{-x} stays within a few per
cent of that where the band-limited Omega rings below zero), plus 2^-22 for the float32 expm1 and the store.  The per-slice sums, fed
with the device's own t and w: |got - want| <= 2 eps sum_r |psi_0|^2 max w, eps = 1e-4 the rel-L2 the parity tests allow the
waves (|psi|^2 moves by 2 eps relative; the wave never gains norm).  Conservation with a whole-plane detector: 2e-4, the same."""
import functools

import numpy as np
import pytest

from oracle import multislice_oracle as orc
from test_gpu_absorptive import EV, U, make_engine, source, stack_from_tables, want

pytestmark = pytest.mark.gpu

GRIDS = [(256, 64, 3), (64, 256, 3), (96, 80, 4), (101, 97, 3)]
PP = [(3.05, 4.4), (1.7, 1.25), (4.1, 2.2)]
DEVICE = 0                                  # (the device of every engine here: Engine's default)
ANNULI = [(40.0, 120.0), (0.0, 40.0), (120.0, 200.0), (20.0, None)]         # mrad


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def detectors(n):
    from pyslice_amd.stem_data import Detector
    return [Detector(f"d{i}", inner=a, outer=b) for i, (a, b) in enumerate(ANNULI[:n])]


def whole_plane():
    from pyslice_amd.stem_data import Detector
    return [Detector("all", inner=0.0)]


def members(dets, w):
    from pyslice_amd.tds import tds_members
    xs, ys = w["xs"], w["ys"]
    return tds_members(dets, len(xs), len(ys), xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV))


@functools.lru_cache(maxsize=None)
def want_tds(nx, ny, nz, n_det):
    """float64: g_det (n_det, 2, nx, ny) in the species order (O, Si) of the device, Omega_det and w (n_det, nz, nx, ny)"""
    from pyslice_amd.tds import tds_tables, tds_weight
    ap, w = source(nx, ny, nz), want(nx, ny, nz)
    xs, ys, zs = w["xs"], w["ys"], w["zs"]
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    q2 = np.fft.fftfreq(nx, dx)[:, None] ** 2 + np.fft.fftfreq(ny, dy)[None, :] ** 2
    bits = members(detectors(n_det), w)
    g, Om = [], []
    for d in range(n_det):
        tabs = {Z: tds_tables(orc.form_factor(q2, Z), q2, U[Z], dx, dy, (bits >> d) & 1) for Z in (8, 14)}
        g.append(np.stack([tabs[8], tabs[14]]))
        Om.append(stack_from_tables(xs, ys, zs, ap.base_positions, np.asarray(ap.atom_types), tabs))
    out = dict(g=np.stack(g), Om=np.stack(Om), w=tds_weight(np.stack(Om), w["sigma"]))
    for v in out.values():
        v.setflags(write=False)
    return out


def resized(ps, grid, dets, **kw):
    """make_engine sizes the handle for test_gpu_absorptive's two probes: this module's three need their own"""
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    ap, w = source(*grid), want(*grid)
    xs, ys, zs = w["xs"], w["ys"], w["zs"]
    kw.setdefault("n_probes", len(PP))
    eng = _native.Engine(len(xs), len(ys), len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], orc.wavelength(EV),
                         orc.interaction_sigma(EV), **kw)
    eng.set_kirkland(ps.loadKirkland())
    eng.set_slices(*slice_edges(zs))
    eng.set_absorption(ap.u_by_Z, True)
    if dets is not None:
        eng.set_tds(members(dets, w), len(dets))
    eng.build_potential(ap.base_positions, ap.atom_types)
    return eng


def propagator(w):
    from pyslice_amd.tilt import tilted_propagator
    xs, ys, zs = w["xs"], w["ys"], w["zs"]
    return tilted_propagator(len(xs), len(ys), xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0], None)


def probes64(w):
    return orc.batched_probes(orc.probe_array(w["xs"], w["ys"], 30.0, EV), w["xs"], w["ys"], PP)


@pytest.mark.parametrize("grid, n_det", [(GRIDS[0], 1), (GRIDS[1], 2), (GRIDS[2], 4), (GRIDS[3], 2)])
def test_tables_and_weights(ps, grid, n_det):
    w, wt = want(*grid), want_tds(*grid, n_det)
    eng = resized(ps, grid, detectors(n_det))
    g = eng.form_factors_tds(2).astype(np.float64)
    W = eng.tds_weight().astype(np.float64)
    a = 2.0 * w["sigma"] ** 2
    for d in range(n_det):
        e_g = np.abs(g[d] - wt["g"][d]).max() / np.abs(wt["g"][d]).max()
        bound_w = a * 1e-5 * np.abs(wt["Om"][d]).max() + 2.0 ** -22
        e_w = np.abs(W[d] - wt["w"][d]).max()
        print(f"tds tables {grid} detector {d}: g_det {e_g:.2e} (1e-5), w {e_w:.2e} (bound {bound_w:.2e}), max w {np.abs(wt['w'][d]).max():.3e}")
        assert e_g <= 1e-5, d
        assert e_w <= bound_w, d
    # the plain absorptive tables next to them are those of a handle without TDS
    plain = make_engine(ps, source(*grid))
    plain.build_potential(source(*grid).base_positions, source(*grid).atom_types)
    assert eng.form_factors_abs(2).tobytes() == plain.form_factors_abs(2).tobytes()
    assert eng.absorption().tobytes() == plain.absorption().tobytes()


@pytest.mark.parametrize("grid, n_det", [(GRIDS[0], 1), (GRIDS[1], 2), (GRIDS[2], 4), (GRIDS[3], 2), (GRIDS[3], 4)])
def test_per_slice_sums_against_the_float64_loop_on_the_device_stacks(ps, grid, n_det):
    """the loop and the reduction alone: tds_signal is fed the device's own t and w"""
    from pyslice_amd.tds import tds_signal
    w = want(*grid)
    eng = resized(ps, grid, detectors(n_det))
    eng.set_probes(30.0, np.asarray(PP))
    eng.propagate()
    got = np.moveaxis(eng.tds_fetch(), 0, -1)                   # (P, D, nz)
    t, W = eng.transmission().astype(np.complex128), eng.tds_weight().astype(np.float64)
    ref, ex = tds_signal(probes64(w), t, W, propagator(w))
    n0 = (np.abs(probes64(w)) ** 2).sum(axis=(1, 2))
    bound = 2.0 * 1e-4 * n0[:, None, None] * np.abs(W).max(axis=(2, 3))[None]
    worst = (np.abs(got - ref) / bound).max()
    print(f"tds per slice {grid} x {n_det}: worst |got - want| / bound {worst:.3e}, of sum |psi0|^2 max w "
          f"{(np.abs(got - ref) / (bound / 2e-4)).max():.3e}")
    assert got.shape == (len(PP), n_det, grid[2])
    assert (np.abs(got - ref) <= bound).all()
    assert np.abs(ref).max() > 1e-6
    # repeats are bitwise equal
    eng.propagate()
    assert np.moveaxis(eng.tds_fetch(), 0, -1).tobytes() == got.tobytes()
    # the stand-alone reduction of the exit waves against slice 0 is the float64 sum of the downloaded waves
    alone, _ = eng.tds_reduce(0, 1)
    ex_dev = eng.exit_waves().astype(np.complex128)
    ref_alone = np.einsum("pxy,dxy->pd", np.abs(ex_dev) ** 2, W[:, 0])
    assert np.abs(alone - ref_alone).max() <= 1e-6 * n0.max() * np.abs(W[:, 0]).max()


def streaming_probe_count(n_tiles, which):
    """A probe count at which the reduction's workgroups stream two or more images each.  The queue halves the images per workgroup
    (pc -> (pc + 1) / 2, from P) until n_tiles * ceil(P / pc) reaches 8 workgroups per CU, so with S = ceil(8 CUs / n_tiles) a count
    of a few S ends above one image.  "odd": 4 S + 1.  "ragged": 8 S - 1, for the devices on which 4 S + 1 happens to be a multiple of
    its chunk (256 CUs: 2049 = 683 * 3 and 2733 = 911 * 3; 4095 = 511 * 8 + 7 and 5463 = 910 * 6 + 3 are not)."""
    import torch
    cus = torch.cuda.get_device_properties(DEVICE).multi_processor_count
    S = -(-8 * cus // n_tiles)
    P = 4 * S + 1 if which == "odd" else 8 * S - 1
    pc = P
    while pc > 1 and n_tiles * -(-P // pc) < 8 * cus:
        pc = (pc + 1) // 2
    print(f"streaming: {cus} CUs, {n_tiles} tiles, P = {P}: {pc} images per workgroup, {P % pc or pc} in the last chunk")
    assert pc >= 2, (cus, P, pc)                                # else the test streams nothing: choose other counts for this device
    assert which != "ragged" or P % pc, (cus, P, pc)
    return P


def check_streaming(eng, reduce, W0, n0):
    """eng has propagated probes whose positions cycle over three, p % 3; reduce = its stand-alone reduction; W0 (n, nx, ny) float64
    the weights of slice 0; n0 the norms of the three probes.  Equal probes give bitwise equal exit waves within a batch, so their
    sums are bitwise equal wherever they stand in a chunk, the short last chunk included."""
    ex = eng.exit_waves()
    bits = ex.view(np.uint64)                                   # (one complex64 pixel)
    for r in range(3):
        assert (bits[r::3] == bits[r]).all(), r
    alone, _ = reduce(0, 1)
    for r in range(3):
        assert (alone[r::3].view(np.uint64) == alone[r].view(np.uint64)).all(), r
    ref = np.einsum("pxy,cxy->pc", np.abs(ex[:3].astype(np.complex128)) ** 2, W0)
    err, bound = np.abs(alone[:3] - ref).max(), 1e-6 * n0.max() * np.abs(W0).max()
    print(f"streaming: |alone - float64 sum| {err:.3e} (bound {bound:.3e}), largest sum {np.abs(ref).max():.3e}")
    assert err <= bound
    assert np.abs(ref).max() > 0
    assert reduce(0, 1)[0].tobytes() == alone.tobytes()


@pytest.mark.parametrize("which", ["odd", "ragged"])
def test_reduction_streams_chunks_of_images_with_a_short_last_chunk(ps, which):
    """96 x 80: 3840 pixel pairs, 4 tiles of 1024 with a partial last one; 4 detectors"""
    grid = GRIDS[2]
    P = streaming_probe_count(4, which)
    eng = resized(ps, grid, detectors(4), n_probes=P)
    eng.set_probes(30.0, np.asarray([PP[p % 3] for p in range(P)]))
    eng.propagate()
    n0 = (np.abs(probes64(want(*grid))) ** 2).sum(axis=(1, 2))
    check_streaming(eng, eng.tds_reduce, eng.tds_weight().astype(np.float64)[:, 0], n0)


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2], GRIDS[3]])
def test_conservation_with_a_whole_plane_detector(ps, grid):
    w = want(*grid)
    eng = resized(ps, grid, whole_plane())
    eng.set_probes(30.0, np.asarray(PP))
    eng.propagate()
    I = eng.tds_fetch()[:, :, 0].sum(axis=0)
    n1 = (np.abs(eng.exit_waves().astype(np.complex128)) ** 2).sum(axis=(1, 2))
    n0 = (np.abs(eng.probes().astype(np.complex128)) ** 2).sum(axis=(1, 2))
    err = np.abs(1.0 - (n1 + I) / n0).max()
    print(f"tds conservation {grid}: |1 - (elastic + tds) / incident| {err:.3e}, tds fraction {(I / n0).max():.4f}")
    assert err <= 2e-4
    assert (I > 1e-4 * n0).all()


def scan(ps, grid, dets, tds, **kw):
    calc = ps.MultisliceCalculator(device=0, progress=False, detectors=dets, tds=tds, **kw)
    calc.setup(source(*grid), aperture=30.0, voltage_eV=EV, probe_positions=PP, sampling=0.1, slice_thickness=1.0)
    return calc, calc.run_detectors()


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[2]])
def test_run_detectors_elastic_part_batches_and_thickness(ps, grid, monkeypatch):
    dets = detectors(2)
    calc, res = scan(ps, grid, dets, True)
    assert res.tds_per_slice.shape == (len(PP), 1, 2, grid[2]) and res.signals.shape == (len(PP), 1, 2)
    # the elastic part: the two-pass loop's, bit for bit; the one-pass loop's within the detectors' bound
    monkeypatch.setenv("MSL_DEBUG", "1")
    monkeypatch.setenv("MSL_SLICE_PATH", "2")
    _, two = scan(ps, grid, dets, False)
    monkeypatch.delenv("MSL_SLICE_PATH")
    monkeypatch.delenv("MSL_DEBUG")
    _, one = scan(ps, grid, dets, False)
    assert res.signals.tobytes() == two.signals.tobytes()
    assert np.abs(res.signals - one.signals).max() <= 2e-4 * one.signals.max()
    assert one.tds_per_slice is None
    # against the engine-level loop
    eng = resized(ps, grid, dets)
    eng.set_probes(30.0, np.asarray(PP))
    eng.propagate()
    npix = float(grid[0] * grid[1])                             # (the units of signals: the unnormalised exit FFT)
    assert np.array_equal(res.tds_per_slice[:, 0], np.moveaxis(eng.tds_fetch(), 0, -1) * npix)
    # elastic and TDS add up in one unit: a whole-plane detector collects the incident beam
    _, full = scan(ps, grid, whole_plane(), True)
    n0 = (np.abs(probes64(want(*grid))) ** 2).sum(axis=(1, 2)) * npix
    err = np.abs(full.total[:, 0, 0] / n0 - 1.0).max()
    print(f"tds run_detectors {grid}: |total / incident - 1| {err:.3e} on a whole-plane detector")
    assert err <= 2e-4
    # a probe batch smaller than the scan: every image is reduced on its own, so the same bits
    _, small = scan(ps, grid, dets, True, probe_batch=2)
    assert small.tds_per_slice.tobytes() == res.tds_per_slice.tobytes()
    assert small.signals.tobytes() == res.signals.tobytes()
    # thickness: the cumulative sums at the entries, next to the elastic series of the same run
    _, thick = scan(ps, grid, dets, True, thickness=[0, 2])
    ks = list(thick.layer)
    assert ks[:2] == [0, 2] and thick.tds.shape == (len(PP), 1, 2, len(ks))
    assert thick.tds_per_slice.tobytes() == res.tds_per_slice.tobytes()
    cum = np.cumsum(res.tds_per_slice, axis=-1)
    for i, k in enumerate(ks):
        assert np.array_equal(thick.tds[..., i], cum[..., k])
    assert np.array_equal(thick.total, thick.signals + thick.tds)
    assert np.abs(thick.signals[..., -1] - res.signals).max() <= 2e-4 * res.signals.max()


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[2]])
def test_clearing_returns_the_handle_to_the_plain_absorptive_run(ps, grid):
    ap = source(*grid)
    eng = resized(ps, grid, detectors(2))
    eng.set_probes(30.0, np.asarray(PP))
    eng.propagate()
    eng.set_tds(None)
    assert eng.buffer_bytes(15) == 0 and eng.buffer_bytes(16) == 0
    with pytest.raises(RuntimeError):
        eng.tds_fetch()
    eng.build_potential(ap.base_positions, ap.atom_types)
    eng.propagate()
    fresh = resized(ps, grid, None)
    fresh.set_probes(30.0, np.asarray(PP))
    fresh.propagate()
    assert eng.exit_waves().tobytes() == fresh.exit_waves().tobytes()
    assert eng.transmission().tobytes() == fresh.transmission().tobytes()
    c0, c1 = eng.counters(), fresh.counters()
    assert c0["algorithmic_bytes"] - c1["algorithmic_bytes"] > 0          # (the TDS loop before the clearing moved more)


def test_set_tds_needs_absorption_and_at_most_four_detectors(ps):
    from pyslice_amd import _native
    grid = GRIDS[2]
    ap, w = source(*grid), want(*grid)
    bits = members(detectors(1), w)
    eng = make_engine(ps, ap, set_abs=False)
    assert eng._lib.msl_set_tds(eng._h, bits.ctypes.data, 1) == _native.MSL_ERR_STATE
    eng.set_absorption(ap.u_by_Z, False)
    assert eng._lib.msl_set_tds(eng._h, bits.ctypes.data, 1) == _native.MSL_ERR_STATE
    eng.set_absorption(ap.u_by_Z, True)
    assert eng._lib.msl_set_tds(eng._h, bits.ctypes.data, 5) == _native.MSL_ERR_INVALID
    eng.set_tds(bits, 1)
    eng.build_potential(ap.base_positions, ap.atom_types)
    assert eng.buffer_bytes(16) == grid[0] * grid[1] * grid[2] * 4
    # another beam: the weights follow sigma, as t does
    from pyslice_amd.tds import tds_weight
    s2 = orc.interaction_sigma(200e3)
    eng.set_beam(orc.wavelength(200e3), s2, 1.0)
    Om = want_tds(*grid, 1)["Om"]
    assert np.abs(eng.tds_weight().astype(np.float64) - tds_weight(Om, s2)).max() <= 2.0 * s2 ** 2 * 1e-5 * np.abs(Om).max() + 2.0 ** -21
    eng.set_absorption(ap.u_by_Z, False)                        # the absorption goes: the TDS with it
    assert eng.buffer_bytes(16) == 0

"""The settings of a handle on the MI355X -- beam (msl_set_beam), tilt (msl_set_tilt), band limit (msl_set_bandlimit) -- and what each
re-derives: the propagator tables, the loop mode and the transmission stacks depend on the settings the
handle ends up with, never on the order they arrived in; a refused call changes nothing; and a handle whose limit is cleared and
that never had a tilt is back on the host tables, through msl_set_beam too.  Through _native.Engine only.

Every assertion is bitwise (array_equal): the six orders launch the same kernels on the same inputs for the state that survives --
tables written from (wavelength, dz, tilt, cuts), stacks made from the resident V with the last sigma and low-passed once with the
last cuts -- and what differs between them (a table or a stack written and overwritten, slices transposed and restored) are copies.
All six orders agree, on both grids and with a resident stack: there is no grouping to report.

nz = 3 (slices of both parities) and 2 probes throughout."""
import itertools

import numpy as np
import pytest

from test_gpu_bandlimit import DZ, EV, _engine, _grid, _positions, _trajectory, white_case

pytestmark = pytest.mark.gpu

EV2 = 200e3                                                                  # the other beam: not the one the handles are created with
ORDERS = list(itertools.permutations(("beam", "tilt", "bandlimit")))
ORDER_IDS = ["-".join(o) for o in ORDERS]


def _beam(eV):
    from pyslice_amd.multislice import interaction_sigma, wavelength
    return wavelength(eV), interaction_sigma(eV), DZ


def _apply(eng, order, tangents, cuts):
    for call in order:
        if call == "beam":
            eng.set_beam(*_beam(EV2))
        elif call == "tilt":
            eng.set_tilt(*tangents)
        else:
            eng.set_bandlimit(*cuts)


def _tangents(tilt_mrad):
    from pyslice_amd.tilt import Tilt
    return tuple(float(t) for t in Tilt(*tilt_mrad).tangents)


# ------------------------------------------------------------------ a. order of the settings, no stack yet
# 96 x 80: the tilt lies along x, a convolution axis, so the loop switches to two-pass; 256 x 64: the planned loop under Tilt(20, -10)
@pytest.mark.parametrize("nx,ny,tilt_mrad", [(96, 80, None), (256, 64, (20.0, -10.0))], ids=["96x80-two-pass", "256x64-planned"])
def test_order_of_the_settings_without_a_stack(nx, ny, tilt_mrad):
    V, psi0, cuts, _ = white_case(nx, ny, 3)
    tangents = (0.01, 0.0) if tilt_mrad is None else _tangents(tilt_mrad)
    runs = []
    for order in ORDERS:
        eng = _engine(nx, ny, 3, 2)
        try:
            _apply(eng, order, tangents, cuts)
            eng.upload_probes(psi0)
            eng.upload_potential(V)
            eng.propagate()
            runs.append((eng.exit_waves().copy(), eng.get_tilt(), eng.get_bandlimit()))
        finally:
            eng.close()
    exit0, tilt0, cuts0 = runs[0]
    assert tilt0 == tangents and cuts0 == cuts
    assert np.isfinite(exit0).all() and np.abs(exit0).max() > 0
    for name, (ex, tilt, cut) in zip(ORDER_IDS, runs):
        assert tilt == tilt0 and cut == cuts0, name
        assert np.array_equal(ex, exit0), name


# ------------------------------------------------------------------ b, c. with a resident stack
def _built_engine():
    """96 x 80 x 3 with keep_potential, built from the synthetic trajectory of test_transmission_stack_in_both_layouts"""
    from pyslice_amd.potentials import loadKirkland, slice_edges
    tr = _trajectory(96, 80, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    assert (len(xs), len(ys), len(zs)) == (96, 80, 3)
    eng = _engine(96, 80, 3, 2, keep_potential=True)
    try:
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(zs))
        eng.build_potential(tr.positions[0], np.asarray(tr.atom_types, dtype=np.int32))
    except Exception:
        eng.close()
        raise
    return eng


def test_order_of_the_settings_with_a_resident_stack():
    """the stack of every order is the one made from the kept V with the last sigma and limited once with the last cuts, in natural
    order on the two-pass loop the tilt along x asks for; V itself is never touched"""
    _, psi0, cuts, _ = white_case(96, 80, 3)
    tangents = (0.01, 0.0)
    runs = []
    for order in ORDERS:
        eng = _built_engine()
        try:
            V0 = eng.potential().copy()
            t0 = eng.transmission().copy()
            _apply(eng, order, tangents, cuts)
            assert np.array_equal(eng.potential(), V0), order
            eng.upload_probes(psi0)
            eng.propagate()
            runs.append((eng.transmission().copy(), eng.exit_waves().copy(), V0, eng.get_tilt(), eng.get_bandlimit()))
        finally:
            eng.close()
    stack0, exit0, V0, tilt0, cuts0 = runs[0]
    assert tilt0 == tangents and cuts0 == cuts
    assert not np.array_equal(stack0, t0)                                    # (another sigma and a limit: not the stack of the build)
    for name, (stack, ex, V, tilt, cut) in zip(ORDER_IDS, runs):
        assert tilt == tilt0 and cut == cuts0, name
        assert np.array_equal(V, V0), name
        assert np.array_equal(stack, stack0), name
        assert np.array_equal(ex, exit0), name


@pytest.mark.parametrize("with_settings", [False, True], ids=["fresh", "tilted-and-limited"])
def test_refused_calls_leave_the_handle_as_it_was(with_settings):
    """after a build and a propagate (and, in the second case, with a tilt, a limit and another beam on the handle, so that there is
    something to put back): a non-finite tangent, cuts that are not alias-free on 96 x 80 (3 * 32 >= 96) and a half-cleared limit"""
    _, psi0, cuts, _ = white_case(96, 80, 3)
    eng = _built_engine()
    try:
        if with_settings:
            _apply(eng, ORDERS[0], (0.01, 0.0), cuts)
        eng.upload_probes(psi0)
        eng.propagate()
        before = (eng.get_tilt(), eng.get_bandlimit(), eng.transmission().copy(), eng.exit_waves().copy())
        assert before[1] == (cuts if with_settings else (-1, -1))
        refused = [lambda: eng.set_tilt(float("nan"), 0.0), lambda: eng.set_bandlimit(32, 4), lambda: eng.set_bandlimit(-1, 4)]
        for i, call in enumerate(refused):
            with pytest.raises(ValueError):
                call()
            assert eng.get_tilt() == before[0], i
            assert eng.get_bandlimit() == before[1], i
            assert np.array_equal(eng.transmission(), before[2]), i
            eng.propagate()
            assert np.array_equal(eng.exit_waves(), before[3]), i
    finally:
        eng.close()


# ------------------------------------------------------------------ d. back to the host tables
def test_back_to_the_host_tables_through_set_beam():
    """test_off_is_off (tests/test_gpu_bandlimit.py) through msl_set_beam: limit set, limit cleared, then the creation beam again --
    a handle that never had a tilt and has no limit writes the tables of msl_create, bit for bit"""
    from pyslice_amd.potentials import loadKirkland, slice_edges
    tr = _trajectory(64, 48, 3, density=0.2)
    xs, ys, zs = _grid(tr)
    Z = np.asarray(tr.atom_types, dtype=np.int32)
    cuts = white_case(64, 48, 3)[2]
    eng = _engine(64, 48, 3, 2)
    try:
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(zs))
        eng.set_probes(30.0, np.asarray(_positions(xs, ys, 2)))
        eng.build_potential(tr.positions[0], Z)
        eng.propagate()
        first = eng.exit_waves().copy()
        eng.set_bandlimit(*cuts)
        eng.set_bandlimit(-1, -1)
        eng.set_beam(*_beam(EV))
        eng.build_potential(tr.positions[0], Z)
        eng.propagate()
        again = eng.exit_waves().copy()
    finally:
        eng.close()
    assert np.isfinite(first).all() and np.abs(first).max() > 0
    assert np.array_equal(again, first)

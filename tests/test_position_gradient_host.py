"""Host checks of the position gradient, no device needed: the float64 definition
(adjoint.position_gradient) against Richardson central differences of the oracle's potential, the chain rule end to end, the calculator
on a recording engine, the ABI, and the yardstick of tests/test_gpu_position_gradient.py -- on exactly its inputs the faults a kernel
can have miss the device bound by a factor 10 and more, and the float32 model of the kernel stays a factor 10 under it.

Measured (white Gamma, flat form factors): max |g| / position_gradient_bound 0.02 .. 0.18 over the cases; the float32 model
(tables, f_Z and B rounded to float32, float64 sums) 1.4e-9 .. 1.0e-8 of the bound, at most 5e-4 of the 2e-5 allowed; every fault at
least 90 x the 2e-5 allowed (the kx / ky swap on the nearly square 101 x 97 grid), the others from 170 x."""
import os
import re

import numpy as np
import pytest

import gradient_cases as gc
import position_gradient_cases as pc
from recording_engine import RecordingEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
orc = gc.orc


# ---- the definition ----
@pytest.mark.parametrize("nx,ny,nz", [(24, 20, 3), (32, 32, 2), (25, 21, 3)])
def test_definition_against_richardson_differences_of_the_oracle(nx, ny, nz):
    from pyslice_amd.adjoint import position_gradient
    rng = np.random.default_rng(nx + ny)
    xs, ys, zs = np.arange(nx) * 0.1, np.arange(ny) * 0.1, np.arange(nz) * 1.0
    n = 12 * nz
    pos = rng.random((n, 3)) * np.array([nx * 0.1, ny * 0.1, nz * 1.0 + 0.3])
    Z = np.array([14, 8])[rng.integers(0, 2, n)]
    gam = rng.standard_normal((nz, nx, ny))
    g = position_gradient(xs, ys, zs, pos, Z, gam)

    def L(p):
        return (gam * np.moveaxis(orc.potential(xs, ys, zs, p, Z), 2, 0)).sum()

    def fd(a, ax, h):
        up, down = pos.copy(), pos.copy()
        up[a, ax] += h
        down[a, ax] -= h
        return (L(up) - L(down)) / (2.0 * h)
    worst = 0.0
    for a in range(0, n, 5):
        for ax in (0, 1):
            worst = max(worst, abs((4.0 * fd(a, ax, 5e-4) - fd(a, ax, 1e-3)) / 3.0 - g[a, ax]) / np.abs(g).max())
    print(f"definition {nx} x {ny} x {nz}: worst |richardson - g| / max |g| {worst:.3e}")
    assert worst <= 1e-8
    outside = pos[:, 2] >= zs[-1] + 1.0
    assert outside.any() and not g[outside].any() and not g[:, 2].any() and g[~outside, :2].all()


def test_slice_axis_zero_restates_the_oracle():
    from pyslice_amd.adjoint import _potential_of, position_gradient
    case = pc.AXIS0
    xs, ys, zs = pc.axes_of(case)
    pos, Z = pc.atoms(case)
    want = np.moveaxis(orc.potential(xs, ys, zs, pos, Z, 0), 2, 0)
    assert np.abs(_potential_of(xs, ys, zs, pos, Z, 0) - want).max() <= 1e-12 * np.abs(want).max()
    g = position_gradient(xs, ys, zs, pos, Z, pc.white_gamma(case), 0)
    assert not g[:, 0].any() and g[:, 1:].all()


@pytest.mark.parametrize("loss", gc.LOSSES)
def test_chain_rule_end_to_end(loss):
    from pyslice_amd.adjoint import position_directional_check
    grid = (32, 24, 2)
    c, tr = gc.case(*grid), gc.trajectory(*grid)
    d = pc.smooth_shift(tr.n_atoms)
    d[:, 2] = 0.0
    kw = dict(loss=loss, epsilon=gc.epsilon_of(c, loss))
    args = (c["xs"], c["ys"], c["zs"], tr.positions[0], tr.atom_types, c["probes"], c["D"], c["sigma"], c["prop"], d)
    (f1, inner), (f2, _) = position_directional_check(*args, 2e-4, **kw), position_directional_check(*args, 1e-4, **kw)
    rich = (4.0 * f2 - f1) / 3.0
    print(f"chain rule {loss}: richardson {rich:.9e} <grad, d> {inner:.9e}")
    assert abs(rich - inner) <= 1e-7 * abs(inner) and inner != 0.0


# ---- the yardstick of the device tests ----
@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_device_bound_sees_every_fault_and_clears_the_float32_model(case):
    want, bound = pc.chain_reference(case)
    assert np.abs(pc.model(case) - want).max() <= 1e-12 * bound.max()               # the model restates the definition
    floor = pc.chain_ratio(case, pc.model(case, float32=True))
    size = np.abs(want[:, pc.in_plane(case)]).max() / bound.max()
    print(f"{case.name}: max |g| / bound {size:.3f}; float32 model / (2e-5 bound) {floor:.3e}")
    assert floor <= 0.1
    for fault in pc.FAULTS:
        if not pc.fault_applies(case, fault):
            continue
        ratio = pc.chain_ratio(case, pc.model(case, fault=fault))
        print(f"{case.name}: fault {fault} / (2e-5 bound) {ratio:.3e}")
        assert ratio >= 10.0, fault


def test_every_fault_is_seen_on_some_case():
    for fault in pc.FAULTS:
        assert any(pc.fault_applies(case, fault) for case in pc.CHAIN_CASES), fault
    assert pc.fault_applies(pc.POW2, "dropped") and pc.fault_applies(pc.GRID_CASES[0], "swap") and pc.fault_applies(pc.POW2, "nyquist_twice")
    pos, Z = pc.atoms(pc.DENSE)
    assert min((Z == 14).sum(), (Z == 8).sum()) >= 128 and (pc.chain_reference(pc.DENSE)[1] > 0).all()      # the padded sf_stream layout, all inside
    pos, Z = pc.atoms(pc.POW2)
    assert not ((Z == 8) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 2.0)).any() and ((Z == 8) & (pos[:, 2] >= 0) & (pos[:, 2] < 0.5)).any()


@pytest.mark.parametrize("grid", pc.RUN_GRIDS)
def test_run_bound_against_the_faults(grid):
    """bound (b) of the device test -- through the L1 -> L2 step of gradient_bound -- on the run's own Gamma: the faults against it"""
    xs, ys, zs = pc.run_axes(grid)                                   # (the calculator's own axes: the box is a hair wider than n x 0.1)
    case = [k for k in pc.GRID_CASES if (k.nx, k.ny, k.nz) == grid][0]._replace(dx=xs[1] - xs[0], dy=ys[1] - ys[0], dz=zs[1] - zs[0])
    ref = pc.run_reference(grid)
    bound_b = pc.run_bound(grid, ref)
    live = ref["bound"][:, 0] > 0
    assert np.abs(pc.model(case, physical=True, gamma=ref["grad"]) - ref["positions"]).max() <= 1e-12 * ref["bound"].max()
    size = (np.abs(ref["positions"][live][:, :2]) / bound_b[live]).max()
    print(f"run {grid}: max |g| / bound (b) {size:.3e}; chain part of (b) / (b) {(pc.CHAIN_TOL * ref['bound'][live] / bound_b[live]).max():.3e}")
    for fault in pc.FAULTS:
        if not pc.fault_applies(case, fault) or fault == "dropped":
            continue
        got = pc.model(case, physical=True, fault=fault, gamma=ref["grad"])
        ratio = (np.abs(got[live][:, :2] - ref["positions"][live][:, :2]) / bound_b[live]).max()
        print(f"run {grid}: fault {fault} / bound (b) {ratio:.3e}")
        # (b) is too loose to ask a factor 10 of every fault -- the L1 -> L2 step through gradient_bound costs about sqrt N, and the
        # gradient itself is only 18 .. 35 bounds: a fault of the size of the gradient (conj(B) -> B, 1 / N) is 10 x and more over
        # it, the other species' table 7.8 x, a wrong slice 2.6 .. 10 x, the 20 % weight swap 1.4 .. 4.9 x, and the Nyquist lines
        # under the physical f_Z (1e-3 of f(0) there) not at all.  Bound (a), the white chain test and the directional derivative
        # are the end-to-end check; (b) stays in the device test as a true but weak bound
        if fault in ("noconj", "no_1_over_N"):
            assert ratio >= 10.0, fault
    assert size >= 10.0                                              # (a result of zeros, or of the wrong sign, misses (b) ten times over)


# ---- calculator logic ----
class PositionRecorder(RecordingEngine):
    def __init__(self, nx, ny, nz, *a, **k):
        super().__init__(nx, ny, nz, *a, **k)
        self._shape, self._n = (nx, ny, nz), 0

    def build_potential(self, positions, Z, slice_axis=2):
        self.calls.append(("build_potential", (positions, Z, slice_axis), {}))
        self._n = len(Z)

    def adjoint_add(self, data, B=None, probe=False):
        self.calls.append(("adjoint_add", (data,), dict(B=B, probe=probe)))
        return np.arange(B, dtype=np.float64) + 1.0, None

    def adjoint_download(self):
        self.calls.append(("adjoint_download", (), {}))
        nx, ny, nz = self._shape
        return np.ones((nz, nx, ny))

    def adjoint_positions(self, gamma=None):
        self.calls.append(("adjoint_positions", (gamma,), {}))
        return np.arange(self._n * 3, dtype=np.float64).reshape(self._n, 3)


@pytest.fixture
def recorder(monkeypatch):
    from pyslice_amd import _native, calculators
    made = []

    def make(*a, **k):
        made.append(PositionRecorder(*a, **k))
        return made[-1]
    monkeypatch.setattr(_native, "Engine", make)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    return made


def setup_calc(ps, recorder, **kw):
    tr = gc.trajectory(96, 80, 4)
    calc = ps.MultisliceCalculator(device=0, progress=False, **kw)
    calc.setup(tr, aperture=30.0, voltage_eV=gc.EV, probe_positions=gc.PP, sampling=0.1, slice_thickness=1.0)
    return calc, recorder[-1], tr


def test_calculator_calls_and_errors(recorder):
    import pyslice_amd as ps
    calc, eng, tr = setup_calc(ps, recorder, gradient=ps.Gradient(positions=True), probe_batch=2)
    eng.calls.clear()
    data = np.ones((3, 96, 80))
    res = calc.run_gradient(data)
    names = [c[0] for c in eng.calls]
    assert names == ["build_potential", "adjoint_reset"] + ["set_probes", "adjoint_add"] * 2 + ["adjoint_download", "adjoint_positions"]
    assert eng.calls[-1][1] == (None,)                               # the accumulator, on the device
    assert res.positions.shape == (tr.n_atoms, 3) and res.positions[2, 1] == 7.0
    assert np.array_equal(res.position_step(np.zeros((tr.n_atoms, 3)), 0.5), -0.5 * res.positions)
    with pytest.raises(ValueError, match="position_step"):
        res.position_step(np.zeros((3, 3)), 0.5)
    eng.calls.clear()
    moved = tr.positions[0] + 0.01
    calc.run_gradient(data, positions=moved)
    assert eng.calls[0][0] == "build_potential" and np.array_equal(eng.calls[0][1][0], moved) and eng.calls[0][1][2] == 2
    with pytest.raises(ValueError, match="potential= does not come from atoms"):
        calc.run_gradient(data, potential=np.zeros((96, 80, 4)))
    with pytest.raises(ValueError, match="positions"):
        calc.run_gradient(data, positions=moved[:5])
    with pytest.raises(ValueError, match="positions"):
        calc.run_gradient(data, positions=np.full(moved.shape, np.nan))
    # Gradient(positions=False): the calls of before, no .positions; positions= still overrides the frame
    calc, eng, tr = setup_calc(ps, recorder, gradient=ps.Gradient(), probe_batch=2)
    eng.calls.clear()
    res = calc.run_gradient(data)
    assert [c[0] for c in eng.calls] == ["build_potential", "adjoint_reset"] + ["set_probes", "adjoint_add"] * 2 + ["adjoint_download"]
    assert res.positions is None
    with pytest.raises(ValueError, match="position_step"):
        res.position_step(moved, 0.5)
    with pytest.raises(ValueError, match="potential= and positions="):
        calc.run_gradient(data, potential=np.zeros((96, 80, 4)), positions=moved)
    assert "positions" not in repr(ps.Gradient()) and "positions=True" in repr(ps.Gradient(positions=True))


def test_definition_argument_checks():
    from pyslice_amd.adjoint import position_gradient, position_gradient_bound
    xs, ys, zs = np.arange(8) * 0.1, np.arange(6) * 0.1, np.arange(2) * 1.0
    pos, Z = np.full((3, 3), 0.2), np.array([14, 8, 14])
    with pytest.raises(ValueError, match="dLdV"):
        position_gradient(xs, ys, zs, pos, Z, np.zeros((8, 6, 2)))
    with pytest.raises(ValueError, match="positions"):
        position_gradient(xs, ys, zs, pos[:, :2], Z, np.zeros((2, 8, 6)))
    with pytest.raises(ValueError, match="slice_axis"):
        position_gradient(xs, ys, zs, pos, Z, np.zeros((2, 8, 6)), slice_axis=3)
    gam = np.random.default_rng(0).standard_normal((2, 8, 6))
    b = position_gradient_bound(xs, ys, zs, pos, Z, gam)
    assert b.shape == (3, 2) and (b > 0).all()
    assert (np.abs(position_gradient(xs, ys, zs, pos, Z, gam)[:, :2]) <= b).all()


# ---- ABI ----
def test_abi():
    from pyslice_amd import _native
    header = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"^int\s+msl_adjoint_positions\(msl_handle\* h, const double\* gamma, double\* out\);", header, re.M)
    assert re.search(r"^int\s+msl_adjoint_positions_time\(msl_handle\* h, int32_t reps, double\* ms_chain\);", header, re.M)
    assert re.search(r"^int64_t msl_adjoint_positions_rows\(const msl_handle\* h\);", header, re.M)
    for name in ("msl_adjoint_positions", "msl_adjoint_positions_rows", "msl_adjoint_positions_time"):
        assert name in _native.EXPORTS
    for name in ("adjoint_positions", "adjoint_positions_time"):
        assert callable(getattr(_native.Engine, name))

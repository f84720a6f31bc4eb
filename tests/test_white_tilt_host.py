"""Host checks of the tilt argument of tools/white_parity.py, the yardstick of tests/test_gpu_white_tilt.py: no device needed.

The tilted float64 reference is pinned three ways -- to the untilted one, to np.roll for a whole-pixel tilt in vacuum, and to an
independent loop on per-axis tables written here -- and faults of the kind a pass kernel can have on a table that is not even in k,
injected into that loop, all exceed the E_img bound of their case.  Measured on the three grids (600 x 135 x 3, 135 x 1728 x 2,
2048 x 144 x 3; E_img of the exit waves over its bound, tangents (0.17, -0.11)):
    table read at -k on one axis           2.3e5 - 3.5e5
    the tilt factor dropped on one axis    2.2e5 - 2.3e5
    Nyquist entry taken at +k, not -k      4.8e3 - 1.2e4
    one entry off by 1e-3 rad              5.5 - 9.5
while the unmutated loop is below 1e-12 of the reference, whatever the order of its transforms.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import rel_l2

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)
orc = wp.orc

LAM, SIGMA = orc.wavelength(wp.EV), orc.interaction_sigma(wp.EV)
MUTANT_GRIDS = [(600, 135, 3), (135, 1728, 2), (2048, 144, 3)]


def axis_table(n, d, tan):
    """the propagator of one axis on the unshifted grid, float64: Fresnel factor times the linear phase of the tilt"""
    k = np.fft.fftfreq(n, d=d)
    return np.exp(-1j * np.pi * LAM * wp.DZ * k ** 2) * np.exp(-2j * np.pi * wp.DZ * k * tan)


def loop(probes, V, px, py, x_first=False):
    """the slice loop on two per-axis tables, one axis at a time (x_first: the other order of the two 1-D transforms)"""
    psi = probes.astype(np.complex128)
    for z in range(V.shape[0]):
        psi = np.exp(1j * SIGMA * V[z].astype(np.float64)) * psi
        if z < V.shape[0] - 1:
            for ax, p in ((1, px[:, None]), (2, py[None, :]))[::1 if x_first else -1]:
                psi = np.fft.ifft(p * np.fft.fft(psi, axis=ax), axis=ax)
    return psi


def test_untilted_reference_is_unchanged():
    nx, ny, nz = 45, 63, 3
    probes, V = wp.white_input(nx, ny, nz, 2)
    xs, ys, zs = np.arange(nx) * wp.DX, np.arange(ny) * wp.DY, np.arange(nz) * wp.DZ
    want = orc.propagate(probes, np.moveaxis(V[0].astype(np.float64), 0, 2), xs, ys, zs, wp.EV)
    for got in (wp.reference(probes, V[0], nx, ny, nz), wp.reference(probes, V[0], nx, ny, nz, tilt=None),
                wp.reference(probes, V[0], nx, ny, nz, tilt=(0.0, 0.0))):
        assert rel_l2(got[0], want) < 1e-14 and rel_l2(got[1], orc.diffraction(want)) < 1e-14
    assert np.array_equal(wp.reference(probes, V[0], nx, ny, nz, tilt=None)[0], want)        # the same call as before
    ex, spec, taps = wp.reference(probes, V[0], nx, ny, nz, layers=(0, 1))
    assert rel_l2(ex, want) < 1e-14 and sorted(taps) == [0, 1]
    t0 = np.exp(1j * SIGMA * V[0, 0].astype(np.float64))
    assert rel_l2(taps[0], orc.diffraction(t0[None] * probes)) < 1e-14


def test_whole_pixel_tilt_in_vacuum_is_a_roll():
    """tangents of +1 px along x and -1 px along y per slice (197 mrad, inside the limit of the small-angle form)"""
    nx, ny, nz = 48, 37, 4
    probes, V = wp.white_input(nx, ny, nz, 2)
    tilt = (wp.DX / wp.DZ, -wp.DY / wp.DZ)
    flat = wp.reference(probes, 0 * V[0], nx, ny, nz)[0]
    got = wp.reference(probes, 0 * V[0], nx, ny, nz, tilt=tilt)[0]
    assert rel_l2(got, np.roll(flat, (nz - 1, -(nz - 1)), axis=(1, 2))) < 1e-12
    assert rel_l2(got, flat) > 1.0
    assert wp.tilt_object(tilt).tangents == pytest.approx(tilt, rel=1e-15) and wp.tilt_object(None).is_zero


@pytest.mark.parametrize("nx,ny,nz,tilt", [(45, 63, 3, wp.TILT), (64, 37, 4, wp.TILT_X), (37, 64, 2, wp.TILT_Y)])
def test_tilted_reference_against_an_independent_loop(nx, ny, nz, tilt):
    probes, V = wp.white_input(nx, ny, nz, 2)
    ex, spec, taps = wp.reference(probes, V[0], nx, ny, nz, tilt=tilt, layers=tuple(range(nz - 1)))
    px, py = axis_table(nx, wp.DX, tilt[0]), axis_table(ny, wp.DY, tilt[1])
    assert rel_l2(ex, loop(probes, V[0], px, py)) < 1e-13 and rel_l2(ex, loop(probes, V[0], px, py, x_first=True)) < 1e-13
    assert rel_l2(spec, np.fft.fftshift(np.fft.fft2(ex), axes=(1, 2))) == 0.0
    assert np.array_equal(ex, wp.reference(probes, V[0], nx, ny, nz, tilt=tilt)[0])
    for k in range(nz - 1):                                   # the tap after slice k is the exit of the first k + 1 slices
        assert rel_l2(taps[k], orc.diffraction(loop(probes, V[0, :k + 1], px, py))) < 1e-13
    # the transposed problem: the other order of the transforms inside fft2
    exT = wp.reference(probes.transpose(0, 2, 1), V[0].transpose(0, 2, 1), ny, nx, nz, tilt=tilt[::-1])[0]
    assert rel_l2(exT.transpose(0, 2, 1), ex) < 1e-12
    assert wp.metrics(ex.astype(np.complex64), ex)[0] < 1e-7           # (the rounding of the result format is far below every bound)


def _mutants(n, table, flat_table):
    """name -> the table of the axis under test with a fault of a pass kernel that an even table hides (the last one excepted)"""
    out = {"read at -k": table[(-np.arange(n)) % n], "tilt factor dropped": flat_table}
    # the Nyquist entry belongs to k = -1 / (2 d) (numpy's fftfreq order); taken at +1 / (2 d) its tilt factor is the conjugate
    f = table.copy(); f[n // 2] = flat_table[n // 2] * np.conj(table[n // 2] / flat_table[n // 2])
    out["Nyquist entry at +k"] = f
    f = table.copy(); f[n // 3] *= np.exp(1e-3j)
    out["one entry off by 1e-3 rad"] = f
    return out


@pytest.mark.parametrize("nx,ny,nz", MUTANT_GRIDS, ids=["x".join(map(str, g)) for g in MUTANT_GRIDS])
def test_faults_on_a_tilted_table_exceed_the_bound(nx, ny, nz):
    probes, V = wp.white_input(nx, ny, nz, 2)
    want = wp.reference(probes, V[0], nx, ny, nz, tilt=wp.TILT)[0]
    bound = wp.bounds(nx, ny, nz, False)[0]
    assert bound == 3e-6 * np.sqrt(2 * (nz - 1))
    px, py = axis_table(nx, wp.DX, wp.TILT[0]), axis_table(ny, wp.DY, wp.TILT[1])
    for x_first in (False, True):
        assert wp.metrics(loop(probes, V[0], px, py, x_first), want)[0] < 1e-12
    along_x = wp.axis_under_test(nx, ny)[0] == nx
    n, d, tan = (nx, wp.DX, wp.TILT[0]) if along_x else (ny, wp.DY, wp.TILT[1])
    assert n % 2 == 0                                                   # (the axis under test has a Nyquist entry)
    hidden = axis_table(n, d, 0.0)
    for name, table in _mutants(n, px if along_x else py, hidden).items():
        e = wp.metrics(loop(probes, V[0], table if along_x else px, py if along_x else table), want)[0]
        print(f"{nx} x {ny} x {nz} {name}: E_img {e:.3e}, {e / bound:.3g} x the bound {bound:.2e}")
        assert e > bound, name
        if name != "one entry off by 1e-3 rad":
            # on the even, untilted table the same fault is no fault at all: what the untilted suites cannot see
            flat = _mutants(n, hidden, hidden)[name]
            assert np.abs(flat - hidden).max() < 1e-12, name


class Float64Engine:
    """the calls white_case() makes of _native.Engine, answered by the loop above in float64, with a fault on request: the plumbing
    of white_case (call order, layer blocks, the restored run) without a device"""

    def __init__(self, nx, ny, nz, P, fault=None, two_pass=False):
        self.shape, self.P, self.fault, self.two_pass = (nx, ny, nz), P, fault, two_pass
        self.tilt, self.layers, self.bytes, self.calls = (0.0, 0.0), [], 0, []

    def upload_probes(self, p):
        self.probes = p

    def upload_potential(self, V):
        self.V = V

    def set_tilt(self, tx, ty):
        self.tilt = (tx, ty)

    def set_layers(self, layers):
        self.layers = list(layers)

    def reset_counters(self):
        self.bytes = 0

    def counters(self):
        return dict(algorithmic_bytes=self.bytes)

    def _loop(self, nz):
        nx, ny, _ = self.shape
        px, py = axis_table(nx, wp.DX, self.tilt[0]), axis_table(ny, wp.DY, self.tilt[1])
        if self.fault == "mirror x":
            px = px[(-np.arange(nx)) % nx]
        return loop(self.probes, self.V[:nz], px, py)

    def propagate(self):
        nx, ny, nz = self.shape
        self.calls.append("propagate")
        self.bytes += (16 * self.P + 8) * nz * nx * ny * (2 if self.two_pass and self.tilt != (0.0, 0.0) else 1)
        self.exit = self._loop(nz).astype(np.complex64)

    def exit_waves(self):
        return self.exit

    def propagate_frame(self, slot):
        self.calls.append("propagate_frame")
        self.blocks = [orc.diffraction(self._loop(k + 1)) for k in self.layers + [self.shape[2] - 1]]

    def wavefunction(self):
        return self.blocks[-1][:, None].astype(np.complex64)

    def layers_c64(self):
        return np.stack(self.blocks)[:, :, None].astype(np.complex64)

    def close(self):
        self.calls.append("close")


def test_white_case_plumbing_on_a_float64_engine(monkeypatch):
    nx, ny, nz, layers = 48, 45, 4, (0, 1, 2)
    made = []

    def fake(fault=None, two_pass=False):
        def make(nx, ny, nz, P, **kw):
            made.append(Float64Engine(nx, ny, nz, P, fault, two_pass))
            return made[-1]
        return make
    monkeypatch.setattr(wp, "tolerance", lambda nx, ny: wp.TOL_DIRECT)         # (no library call: both lengths are 13-smooth)
    monkeypatch.setattr(wp, "engine", fake())
    res = wp.white_case(nx, ny, nz, tilt=wp.TILT, layers=layers)
    assert made[-1].calls == ["propagate", "propagate_frame", "propagate_frame", "close"] and res["one_pass"]
    assert max(res["exit"][0], res["spectrum"][0], res["layers_exit"][0]) < 2e-7 and res["moved"] > 1.0
    for k in layers:
        assert res["layers"][k][0] < 2e-7
        assert (res["layers_moved"][k] > 1.0) == (k > 0)
    assert all(v <= b for v, b in zip(res["layers_untilted"][0], wp.bounds(nx, ny, nz, True, layer=0)))
    assert res["layers_untilted"][1][0] > 1.0
    untilted = wp.white_case(nx, ny, nz)
    assert untilted["one_pass"] and untilted["exit"][0] < 2e-7 and "moved" not in untilted
    # a table read at -k: every tilted result is off by about sqrt 2, the tap after slice 0 (nothing propagated yet) is not
    monkeypatch.setattr(wp, "engine", fake("mirror x"))
    res = wp.white_case(nx, ny, nz, tilt=wp.TILT, layers=layers)
    assert min(res["exit"][0], res["spectrum"][0], res["layers"][1][0], res["layers"][2][0], res["layers_exit"][0]) > 1.0
    assert res["layers"][0][0] < 2e-7
    assert wp.white_case(nx, ny, nz)["exit"][0] < 2e-7                    # ... and without a tilt the fault is invisible
    # a tilt that takes the two-pass loop, and (0, 0) on the same engine
    monkeypatch.setattr(wp, "engine", fake(two_pass=True))
    res = wp.white_case(nx, ny, nz, tilt=wp.TILT_X, restore=True)
    assert not res["one_pass"] and res["restored"]["one_pass"] and res["moved"] > 1.0
    assert res["exit"][0] < 2e-7 and res["restored"]["exit"][0] < 2e-7 and res["restored"]["spectrum"][0] < 2e-7


def test_tap_axis_restates_the_slice_order_of_the_loop():
    """mslice.hip, slice_is_transposed: two four-step axes alternate so that the LAST pass runs along y, every other pair of
    kinds starts along y; the tap after slice k reads the pass of slice k"""
    assert [wp.tap_axis(600, 135, 4, k) for k in range(3)] == ["y", "x", "y"]
    assert [wp.tap_axis(1024, 144, 4, k) for k in range(3)] == ["y", "x", "y"]
    assert [wp.tap_axis(256, 256, 4, k) for k in range(3)] == ["x", "y", "x"]
    assert [wp.tap_axis(256, 1024, 3, k) for k in range(2)] == ["y", "x"]
    assert wp.tap_axis(501, 144, 4, 1, one_pass=False) == "two-pass"
    src = open(os.path.join(os.path.dirname(__file__), "..", "pyslice_amd", "csrc", "mslice.hip")).read()
    assert "return h->scheme_b ? ((s & 1) != 0) : (((h->cfg.nz - 1 - s) & 1) != 0);" in src
    assert "h->scheme_b = h->onepass && !(h->opx.kind == AX_FOURSTEP && h->opy.kind == AX_FOURSTEP);" in src

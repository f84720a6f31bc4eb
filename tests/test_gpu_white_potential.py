"""White-spectrum parity of the potential build, per image, per k-bin, per k-line and per pixel (tools/white_potential.py).

The physical-table potential tests bound max|dV| / max|V|: Kirkland form factors fall off steeply and max|V| is the peak at an atom,
so a single mirrored bin, a tile corner or an edge-kernel lane that is 50 % wrong at high k passes them on the 512^2 .. 2048^2 grids
(tests/test_white_potential_host.py states that as a checked fact).  Here the form factors are flat -- B, N, Si = 1, -0.7, 0.45, Si
with a Gaussian a factor 2 down at the corner of k-space, dx = 0.1, dy = 0.09 -- so R_s is white and every bin of every structure-
factor kernel and every line of every inverse-transform form carries the same weight.  The transmission functions (sigma =
0.3 / rms V) and, with keep_potential, the potential itself are compared with the float64 formula through
dV = Im(t conj t_want) / sigma and D = fft2(dV) dx^2 dy^2:
    E_img <= tol, E_kline <= 2 tol, E_bin <= 10 tol, E_pix <= 10 tol + 2^-24 max|sigma V| / 0.3, E_mod <= 4 x 2^-24,
tol = 3e-6 where both axes of the inverse transform run a direct kernel, 1e-5 where one runs chirp-z or a Bluestein plan: the
white-noise contract of test_fft2_matches_numpy for the one 2-D transform of the build; a slice without atoms is |t - 1| <= 2^-23.
Every id carries the label of white_potential.path(): the form of plan_pot_ifft with the kernel of the y and of the x pass, and the
structure-factor kernel with its edge kernel; path()'s view of the slice loop is checked against the engine's byte counter.
Found by it: 2048 x 2048 x 3 sparse (PI_WAVE2K) had E_pix 4.69e-5 against 4.39e-5, with E_bin 0.04 and E_kline 0.05 of their bounds --
no bin or line at fault, a pixel with a phase of 70 rad: the epilogue of the transposing forms multiplied by two separately rounded
constants (scale, sigma / pi), each rounding 2^-24 of the phase.  ifft_transposed now passes their product, formed in double and
rounded once: E_pix 3.58e-5, E_bin 1.15e-6, E_kline 2.5e-7 after (1.22e-6 and 2.8e-7 before).
Run on the MI355X box with `pytest -m gpu`; `python tools/white_potential.py profiles/white_potential_parity.txt` records the
measured figures per kernel family (a record: the bounds are not taken from it).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("white_potential", os.path.join(os.path.dirname(__file__), "..", "tools", "white_potential.py"))
wpot = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wpot)

_RAW = {}            # transmission functions of the runs without a debug switch, for the runs that must differ from them


def _ids(cases):
    return [wpot.case_id(c) for c in cases]


def _run(c, monkeypatch):
    if c.env:
        monkeypatch.setenv("MSL_DEBUG", "1")
        for name in c.env:
            monkeypatch.setenv(name, "1")
    res = wpot.white_potential_case(c)
    b, p = res["bounds"], wpot.case_path(c)
    runs = [(f"slot {i}", m) for i, m in enumerate(res["t"])] + ([("potential()", res["V"])] if res["V"] else [])
    for what, m in runs:
        print(f"{wpot.case_id(c)} {what}: " + " ".join(f"{k} {m[k]:.3e} ({m[k] / b[k]:.2f})" for k in wpot.METRICS) +
              f" E_empty {m['E_empty']:.1e} | bin {m['bin']} line {m['line']}")
    assert res["one_pass"] == p.one_pass, "path() and the engine disagree on the slice loop of this grid"
    for what, m in runs:
        for k in wpot.METRICS + ("E_empty",):
            assert m[k] <= b[k], f"{what} {k} {m[k]:.3e} above {b[k]:.3e} (bin {m['bin']}, line {m['line']})"
    if not c.env and c.batch == 1 and c.kind == "uniform" and not c.keep and c.fft_path == 0:
        _RAW[c] = res["raw"][0]
    return res


def _against_default(c, res, monkeypatch):
    """the raw transmission functions of the same case without its switch, and of this run"""
    d = c._replace(env=())
    if d not in _RAW:
        monkeypatch.delenv("MSL_DEBUG", raising=False)
        _run(d, monkeypatch)
    assert res["raw"][0].shape == _RAW[d].shape
    return _RAW[d].view(np.uint32), res["raw"][0].view(np.uint32)


@pytest.mark.parametrize("c", wpot.SF_CASES, ids=_ids(wpot.SF_CASES))
def test_structure_factor_kernels(c, monkeypatch):
    """quad (sparse), stream_bf16 (dense), stream (MSL_SF_F32), bf16x2 (MSL_SF_TWO_TILES; 96 x 80 and 320 x 200: the second tile of
    the last pair stores nothing; 2048^2 takes it by itself) under the same four-step inverse transform where the grid allows"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.EDGE_CASES, ids=_ids(wpot.EDGE_CASES))
def test_nyquist_rows_and_columns(c, monkeypatch):
    """structure_factor_edge_kernel on x only, on y only, on both (the corner bin), on neither, and odd lengths without a Nyquist bin"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.ROWS_CASES, ids=_ids(wpot.ROWS_CASES))
def test_full_rows(c, monkeypatch):
    """write_mx = 1: all four mirror images stored by the structure-factor kernels (keep_potential, the two-pass engine)"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.LINES_CASES, ids=_ids(wpot.LINES_CASES))
def test_inverse_transform_in_place(c, monkeypatch):
    """PI_LINES: four-step Hermitian columns, out_real + transpose_odd_slices (keep_potential), generic and Bluestein lines, a
    1025 .. 2047-point axis; the grids whose planned form is another one are labelled with it"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.CHIRPZ16_CASES + wpot.CHIRPZ32_CASES + wpot.CHIRPZ64_CASES,
                         ids=_ids(wpot.CHIRPZ16_CASES + wpot.CHIRPZ32_CASES + wpot.CHIRPZ64_CASES))
def test_inverse_transform_chirpz(c, monkeypatch):
    """PI_CHIRPZ with R = 16, 32 (135 and 491 lines: ragged last items of the two-line first and the paired second pass) and 64
    (range ends, a mixed-radix length, a prime, a power of two next to a convolution axis)"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.CHIRPZ32_SWITCH_CASES + wpot.TWO_CASES[2:], ids=_ids(wpot.CHIRPZ32_SWITCH_CASES + wpot.TWO_CASES[2:]))
def test_inverse_transform_without_two_line_and_paired_passes(c, monkeypatch):
    """the one-line first pass and the unpaired second pass meet the same bounds.  The unpaired pass (one complex transform per
    line instead of one per two real lines) differs bit-wise from the default run: the switch took effect.  The one-line first pass
    does not and cannot: ifftTB_two_kernel runs ifftTB_kernel<32>'s instruction sequence on each of its two lines and differs in the
    tile round only, so the two are the same numbers (measured: identical on 501 x 491 x 3) -- asserted as equality, which checks the
    two-line kernel's tile and ragged last item (251 rows of 491 points) against the one-line kernel bit for bit"""
    res = _run(c, monkeypatch)
    default, got = _against_default(c, res, monkeypatch)
    if c.env == wpot.NO_TWO_LINE:
        assert np.array_equal(got, default)
    else:
        assert not np.array_equal(got, default)


@pytest.mark.parametrize("c", wpot.TWO_CASES[:2] + wpot.WAVE2K_CASES, ids=_ids(wpot.TWO_CASES[:2] + wpot.WAVE2K_CASES))
def test_inverse_transform_512_and_2048(c, monkeypatch):
    """PI_TWO (ifftT2_kernel) at both depths, PI_WAVE2K (ifftTW_kernel) at nz = 3 (nz = 2 is the dense structure-factor case)"""
    _run(c, monkeypatch)


@pytest.mark.parametrize("c", wpot.BATCH_CASES, ids=_ids(wpot.BATCH_CASES))
def test_frames_per_launch(c, monkeypatch):
    """build_potentials with nz = 3: from the second frame on the image index and the slice index differ in parity (slice_mod);
    every slot against its own reference, and slot 0 is not slot 1: |t_0 - t_want,1| / |t_want,1 - 1| > 1 (about sqrt 2; E_img
    itself saturates at the atoms of a spiky potential and is 0.45 .. 0.76 between two float64 references)"""
    res = _run(c, monkeypatch)
    print(f"slot 0 against the reference of slot 1: {res['cross']:.3f}")
    assert res["cross"] > 1.0


@pytest.mark.parametrize("c", wpot.ATOM_CASES, ids=_ids(wpot.ATOM_CASES))
def test_atoms_at_the_edges(c, monkeypatch):
    """an empty middle slice, a slice with one species, a slice with one atom on a grid point, atoms at 0 and at L - 1e-9, outside
    the box on both sides, outside every slice, and the two other slice axes"""
    _run(c, monkeypatch)

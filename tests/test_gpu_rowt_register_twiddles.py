"""The transposing pass of 1024-point lines with half of its inter-FFT twiddles in registers (rowt_pass.h), through the
calculator's engine against the oracle, with the residual metric and the tolerances of the g6 / one-pass tests of test_gpu_parity.py.

Which instantiations of rowT_pass_kernel<32, 16, IN_P, OUT_P, FL> a stack of nz slices on a 1024 x 1024 grid launches (the last slice
is the in-place pass of another kernel): pass 0 <0,1,2>, passes 1 .. nz - 3 <1,1,3>, pass nz - 2 <1,0,3>.  Three slices therefore run
<0,1,2> and <1,0,3>; four slices add <1,1,3>, the kernel of every middle pass; four slices without the interleaved line order run
<0,0,3> and the run-time-flag form <0,0,-1>, which keeps every twiddle in the table.  <1,0,1>, the ending of stacks whose last pass
transposes, is not reached from a 1024 x 1024 grid and has no case here.  Fewer probes than a probe chunk: the chunk's tail and the
prefetch past the last work item run as well.  The 256-point kernel (R = 16) keeps its table path and has no case here."""
import numpy as np
import pytest

from conftest import rel_l2, ref_residual

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4
RESID_TOL = 1e-6


def npy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@pytest.mark.parametrize("frames,P,fb,nz,interleave", [(1, 2, 1, 3, True), (2, 3, 2, 3, True), (1, 2, 1, 4, True), (1, 2, 1, 4, False)])
def test_1024_grid_vs_oracle(frames, P, fb, nz, interleave, monkeypatch):
    """frame batch 1 with 2 probes; frame batch 2 with 3 probes (per-frame transmission stacks inside one launch, odd image count);
    four slices with and without the interleaved line order between the passes"""
    import pyslice_amd as ps
    from pyslice_amd.synthetic import synthetic_trajectory
    from oracle import multislice_oracle as orc
    if not interleave:
        monkeypatch.setenv("MSL_DEBUG", "1")
        monkeypatch.setenv("MSL_NO_INTERLEAVE", "1")
    n = 1024
    tr = synthetic_trajectory(n, nz, frames, density=0.05, seed=57 + frames + nz)
    lx, ly = tr.box_matrix[0, 0], tr.box_matrix[1, 1]
    pp = [tuple(v) for v in np.random.default_rng(5).random((P, 2)) * [lx, ly]]
    calc = ps.MultisliceCalculator(progress=False, dtype="complex64", frame_batch=fb)
    calc.setup(tr, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert (calc.nx, calc.ny, calc.nz) == (n, n, nz)
    assert calc._engine.frame_batch == fb
    got = npy(calc.run().wavefunction_data)
    want = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 30.0, 100e3, pp)["wavefunction_data"]
    err, res = rel_l2(got, want), ref_residual(got, want)
    print(f"frames {frames} probes {P} frame_batch {fb} slices {nz} interleave {interleave}: rel-L2 {err:.3e}, residual {res:.3e}")
    assert err < WAVE_TOL
    assert res < RESID_TOL

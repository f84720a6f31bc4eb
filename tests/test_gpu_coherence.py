"""Partial coherence on the MI355X: the member probes of msl_set_probe_members against float64 NumPy, msl_diffract_members against
the host fold of msl_diffract's own output (bit for bit) and against float64 NumPy, msl_dose_add_members and the draw from it, and
the calculator's three scan modes with a Coherence against a host fold of G plain scans.

End to end: 64 x 64 pixels of 0.1 A, 4 slices, 2 frames, 4 positions, a defocused, Cs-aberrated 25 mrad probe at 100 kV,
Coherence(focal_spread=40, focal_points=3, source_size=0.3, source_points=3): G = 27."""
import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_aberrations import PROBE_TOL, WAVE_TOL, all_terms, numpy_probes

pytestmark = pytest.mark.gpu

EV = 100e3
ORDER = ["C10", "C12", "C21", "C23", "C30", "C32", "C34", "C41", "C43", "C45", "C50", "C52", "C54", "C56"]


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def with_defocus(ps, ab, d):
    """the Aberrations `ab` (None: none) with C10 + d"""
    p = np.zeros((14, 2)) if ab is None else np.array(ab.as_polar(), dtype=np.float64)
    kw = {}
    for (c, phi), name in zip(p, ORDER):
        kw[name] = c
        if name[2] != "0":
            kw["phi" + name[1:]] = phi
    kw["C10"] = kw["C10"] + d
    return ps.Aberrations(**kw)


# ------------------------------------------------------------------ 1. member probes
OFFSETS = (0.0, 37.5, -37.5, 80.0, -12.3, 0.0)


@pytest.mark.parametrize("tag", ["64", "75x63"])
@pytest.mark.parametrize("aberrated", [False, True], ids=["plain", "14terms"])
def test_member_probes_match_numpy(ps, tag, aberrated):
    from pyslice_amd import _native
    xs, ys = (np.arange(64) * 0.1, np.arange(64) * 0.1) if tag == "64" else (np.arange(75) * 0.1, np.arange(63) * 0.11)
    mrad = 30.0
    lx, ly = len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])
    pp = [tuple(v) for v in np.random.default_rng(5).random((6, 2)) * [lx, ly]]
    ab = all_terms(ps) if aberrated else None
    eng = _native.Engine(len(xs), len(ys), 1, xs[1] - xs[0], ys[1] - ys[0], 0.5, ps.wavelength(EV), 0.0, n_probes=6, n_frames=0)
    try:
        eng.set_aberrations(ab)
        eng.set_probe_members(mrad, pp, OFFSETS)
        got = eng.probes()
        for p, d in enumerate(OFFSETS):
            want = numpy_probes(ps, xs, ys, mrad, EV, with_defocus(ps, ab, d), positions=[pp[p]])[0]
            err = rel_l2(got[p], want)
            print(f"grid {tag} {'14 terms' if aberrated else 'plain'} probe {p} defocus {d:+g}: rel-L2 {err:.3e}")
            assert err <= PROBE_TOL
        assert not np.array_equal(got[1], got[2])
        # every offset zero: msl_set_probes, bit for bit
        eng.set_probes(mrad, pp)
        plain = eng.probes()
        eng.set_probe_members(mrad, pp, np.zeros(6))
        assert np.array_equal(eng.probes(), plain)
        # the probes with offset 0 of the mixed call agree with it too, to the bound (another kernel when the handle has no terms)
        assert rel_l2(got[0], plain[0]) <= PROBE_TOL and rel_l2(got[5], plain[5]) <= PROBE_TOL
        for bad in (dict(mrad=0.0, d=OFFSETS), dict(mrad=mrad, d=(0.0, np.nan, 0.0, 0.0, 0.0, 0.0)),
                    dict(mrad=mrad, d=(0.0, np.inf, 0.0, 0.0, 0.0, 0.0)), dict(mrad=-1.0, d=OFFSETS)):
            with pytest.raises(ValueError):
                eng.set_probe_members(bad["mrad"], pp, bad["d"])
        df = np.zeros(5)
        assert eng._lib.msl_set_probe_members(eng._h, mrad, _native._ptr(np.zeros((5, 2))), _native._ptr(df), 5) == _native.MSL_ERR_INVALID
        eng.set_probes(mrad, pp)                                              # a refused call leaves the handle usable
        assert np.array_equal(eng.probes(), plain)
    finally:
        eng.close()


@pytest.mark.parametrize("tag", ["64", "75x63"])
def test_one_defocus_on_every_member_is_set_probes_at_that_c10(ps, tag):
    """msl_set_probe_members with one non-zero defocus d on every probe against msl_set_probes with C10 + d, all 14 terms non-zero:
    the same kernel body with the C10 coefficient (C10 + d) / (2 lambda) from the device array or from the handle -- bit for bit"""
    from pyslice_amd import _native
    xs, ys = (np.arange(64) * 0.1, np.arange(64) * 0.1) if tag == "64" else (np.arange(75) * 0.1, np.arange(63) * 0.11)
    mrad, d = 30.0, 37.5
    lx, ly = len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])
    pp = [tuple(v) for v in np.random.default_rng(7).random((3, 2)) * [lx, ly]]
    assert len(set(pp)) == 3
    ab = all_terms(ps)
    assert np.all(ab.as_polar()[:, 0] != 0)
    eng = _native.Engine(len(xs), len(ys), 1, xs[1] - xs[0], ys[1] - ys[0], 0.5, ps.wavelength(EV), 0.0, n_probes=3, n_frames=0)
    try:
        eng.set_aberrations(ab)
        eng.set_probe_members(mrad, pp, np.full(3, d))
        members = eng.probes()
        eng.set_aberrations(with_defocus(ps, ab, d))
        eng.set_probes(mrad, pp)
        plain = eng.probes()
        assert not np.array_equal(members[0], members[1])
        assert np.array_equal(members, plain)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. msl_diffract_members
def block_sum(I, bx, by):
    wx, wy = I.shape[-2:]
    return I.reshape(I.shape[:-2] + (wx // bx, bx, wy // by, by)).sum(axis=(-3, -1))


def _engine(wx, wy):
    from pyslice_amd import _native
    return _native.Engine(wx, wy, 1, 0.1, 0.1, 1.0, 0.037, 0.0, n_probes=1, n_frames=0, device=0)


def _weights(G):
    x, w = np.polynomial.hermite.hermgauss(G)
    return w / np.sqrt(np.pi) if G > 1 else np.array([1.0])


T_ROWS = 10
MEMBER_CASES = [
    # (wx, wy), ld pad, bins
    ((16, 16), 0, [(1, 1), (2, 2), (4, 2)]),                    # 16-byte loads: DIRECT, SHFL
    ((15, 21), 0, [(1, 1), (3, 7), (5, 3)]),                    # odd wy: 8-byte loads: DIRECT, LDS
    ((12, 20), 5, [(1, 1), (2, 2), (4, 2), (3, 5)]),            # odd pitch: 8-byte loads: DIRECT, SHFL, LDS
    ((12, 20), 0, [(2, 2), (3, 5)]),                            # 16-byte loads: SHFL, LDS
]


@pytest.fixture(scope="module")
def member_waves():
    """random complex64 (15, T_ROWS, K) per case, amplitudes over 4.5 decades per (wave, frame) -- made once, left unchanged"""
    out = {}
    for (wx, wy), pad, _ in MEMBER_CASES:
        rng = np.random.default_rng(wx * 100 + wy + pad)
        K = wx * wy
        W = (rng.standard_normal((15, T_ROWS, K)) + 1j * rng.standard_normal((15, T_ROWS, K))).astype(np.complex64)
        W *= rng.choice([1e-3, 1.0, 30.0], size=(15, T_ROWS, 1)).astype(np.float32)
        out[(wx, wy, pad)] = W
    return out


@pytest.mark.parametrize("shape,ld_pad,bins", MEMBER_CASES)
def test_diffract_members_is_the_fold_of_diffract(ps, member_waves, shape, ld_pad, bins):
    import torch
    from pyslice_amd.coherence import fold_members
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    W = member_waves[(wx, wy, ld_pad)]
    host = np.full((15, T_ROWS, ld), np.nan + 1j * np.nan, dtype=np.complex64)       # pad pixels must never be read
    host[:, :, :K] = W
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    I = (np.abs(W.astype(np.complex128)) ** 2).reshape(15, T_ROWS, wx, wy)
    eng = _engine(wx, wy)
    worst = 0.0
    try:
        for G in (1, 3, 5):
            w = _weights(G)
            if G > 1:
                assert len(set(w.tolist())) > 1                                      # unequal weights
            for Q in (1, 3):
                B = Q * G
                src = (dW.data_ptr(), B, T_ROWS, wx, wy, ld)
                for bx, by in bins:
                    for count in (1, 3, 9):
                        got = eng.diffract_members(w, t0=1, count=count, bin=(bx, by), src=src)
                        assert got.shape == (Q, wx // bx, wy // by) and got.dtype == np.float64
                        per_wave = eng.diffract(t0=1, count=count, bin=(bx, by), src=src)
                        assert np.array_equal(got, fold_members(per_wave, w)), (G, Q, bx, by, count)
                        if G == 1:
                            assert np.array_equal(got, per_wave)
                        want = np.einsum("g,qgxy->qxy", w, block_sum(I[:B, 1:1 + count].sum(axis=1), bx, by).reshape(Q, G, wx // bx, wy // by))
                        err = (np.abs(got - want) / want).max()
                        worst = max(worst, err)
                        assert err <= 1e-6, (G, Q, bx, by, count, err)
                        assert np.array_equal(eng.diffract_members(w, t0=1, count=count, bin=(bx, by), src=src), got)
        print(f"window {shape} ld+{ld_pad}: worst relative error against float64 NumPy {worst:.3e}")
    finally:
        eng.close()


def test_many_strips_share_a_workgroup(ps):
    """131 positions x 63 rows of bins = 8253 strips: above 8192 the launch gives a workgroup two strips (the last one a single
    strip), in the plain and in the accumulating form"""
    import torch
    from pyslice_amd.coherence import fold_members
    Q, G, T, wx, wy = 131, 3, 2, 63, 4
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((Q * G, T, wx * wy)) + 1j * rng.standard_normal((Q * G, T, wx * wy))).astype(np.complex64)
    dW = torch.from_numpy(W).cuda()
    torch.cuda.synchronize()
    w = _weights(G)
    eng = _engine(wx, wy)
    try:
        src = (dW.data_ptr(), Q * G, T, wx, wy)
        for bin in ((1, 1), (1, 2), (1, 4)):
            got = eng.diffract_members(w, bin=bin, src=src)
            assert got.shape == (Q, wx, wy // bin[1])
            assert np.array_equal(got, fold_members(eng.diffract(bin=bin, src=src), w)), bin
            want = np.einsum("g,qgxy->qxy", w, block_sum((np.abs(W.astype(np.complex128)) ** 2).sum(axis=1).reshape(Q, G, wx, wy), *bin))
            assert (np.abs(got - want) / want).max() <= 1e-6
            eng.dose_reset(Q, got.shape[1:])
            eng.dose_add_members(w, bin=bin, src=src)
            eng.dose_add_members(w, bin=bin, src=src)
            assert np.array_equal(eng.dose_counts(0.0, 1, B=Q, keep_intensity=True)[1], got + got)
    finally:
        eng.close()


def test_diffract_members_refusals(ps):
    import torch
    from pyslice_amd import _native
    eng = _engine(6, 8)
    try:
        d = torch.zeros((6, 3, 50), dtype=torch.complex64, device="cuda")
        p = d.data_ptr()
        w3 = _weights(3)
        ok = (p, 6, 3, 6, 8, 50)
        assert eng.diffract_members(w3, bin=(3, 4), src=ok).shape == (2, 2, 2)
        for w, kw in ((w3, dict(src=(p, 5, 3, 6, 8, 50))),                    # B is no multiple of G
                      (w3, dict(src=(p, 0, 3, 6, 8, 50))),
                      (np.zeros(0), dict(src=ok)),                            # G = 0
                      (np.full(129, 1.0 / 129), dict(src=(p, 129, 3, 6, 8, 50))),      # G above MSL_MEMBERS_MAX (refused before any read)
                      (np.array([0.5, -0.1, 0.6]), dict(src=ok)),
                      (np.array([0.5, np.nan, 0.5]), dict(src=ok)),
                      (np.array([0.5, np.inf, 0.5]), dict(src=ok)),
                      (w3, dict(bin=(4, 1), src=ok)),                         # what msl_diffract refuses
                      (w3, dict(bin=(1, 3), src=ok)),
                      (w3, dict(bin=(0, 1), src=ok)),
                      (w3, dict(src=(p, 6, 3, 6, 8, 47))),
                      (w3, dict(t0=2, count=2, src=ok)),
                      (w3, dict(t0=-1, count=1, src=ok)),
                      (w3, dict(t0=0, count=0, src=ok))):
            with pytest.raises(ValueError):
                eng.diffract_members(w, **kw)
            eng.dose_reset(2, (6, 8))
            with pytest.raises(ValueError):
                eng.dose_add_members(w, **kw)
        out = np.empty(8, dtype=np.float64)
        lib, h = eng._lib, eng._h
        assert lib.msl_diffract_members(h, p, 6, 3, 47, 50, 0, 1, 6, 8, 3, 4, 3, _native._ptr(w3), _native._ptr(out)) == _native.MSL_ERR_INVALID
        assert lib.msl_diffract_members(h, p, 6, 3, 48, 50, 0, 1, 6, 8, 3, 4, 3, None, _native._ptr(out)) == _native.MSL_ERR_INVALID
        assert lib.msl_diffract_members(h, p, 6, 3, 48, 50, 0, 1, 6, 8, 3, 4, 3, _native._ptr(w3), None) == _native.MSL_ERR_INVALID
        with pytest.raises(RuntimeError):
            eng.diffract_members(w3)                                          # no wavefunction ring: MSL_ERR_STATE
        # the accumulator: a state error before the reset, positions beyond it, another pattern shape
        eng2 = _engine(6, 8)
        try:
            with pytest.raises(RuntimeError):
                eng2.dose_add_members(w3, bin=(3, 4), src=ok)
            eng2.dose_reset(1, (2, 2))
            with pytest.raises(ValueError):
                eng2.dose_add_members(w3, bin=(3, 4), src=ok)                 # 2 positions, sized for 1
            eng2.dose_reset(2, (6, 8))
            with pytest.raises(ValueError):
                eng2.dose_add_members(w3, bin=(3, 4), src=ok)                 # 2 x 2 pixels, sized for 6 x 8
        finally:
            eng2.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. msl_dose_add_members
@pytest.mark.parametrize("shape,ld_pad,bin,G", [((16, 16), 0, (2, 2), 3), ((15, 21), 0, (3, 7), 5), ((12, 20), 5, (1, 1), 3),
                                                ((12, 20), 0, (3, 5), 5)])
def test_dose_add_members_accumulates_and_draws(ps, member_waves, shape, ld_pad, bin, G):
    import torch
    wx, wy = shape
    K, ld = wx * wy, wx * wy + ld_pad
    Q = 3
    host = np.zeros((Q * G, T_ROWS, ld), dtype=np.complex64)
    host[:, :, :K] = member_waves[(wx, wy, ld_pad)][:Q * G]
    dW = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    w = _weights(G)
    eng = _engine(wx, wy)
    try:
        src = (dW.data_ptr(), Q * G, T_ROWS, wx, wy, ld)
        mx, my = wx // bin[0], wy // bin[1]
        want = eng.diffract_members(w, 0, 4, bin=bin, src=src) + eng.diffract_members(w, 4, 6, bin=bin, src=src)
        eng.dose_reset(Q + 1, (mx, my))                                       # (sized for more positions than are added)
        eng.dose_add_members(w, 0, 4, bin=bin, src=src)
        eng.dose_add_members(w, 4, 6, bin=bin, src=src)
        counts, acc = eng.dose_counts(0.05, 77, probe0=1000, B=Q, keep_intensity=True)
        assert acc.shape == (Q, mx, my) and np.array_equal(acc, want)
        lam = acc * 0.05
        ref = ps.poisson_counts(lam, 77, 1000 + np.arange(Q))
        differ = int((ref != counts).sum())
        print(f"window {shape} bin {bin} G {G}: lam in [{lam.min():.3e}, {lam.max():.3e}], {differ} of {lam.size} counts differ")
        assert differ <= max(1, int(1e-4 * lam.size))
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. end to end
MRAD = 25.0
C10, CS = -150.0, 2.0e6
PP = [(1.3, 2.1), (3.2, 3.2), (4.05, 0.7), (5.9, 5.1)]


def _coherence(ps):
    return ps.Coherence(focal_spread=40.0, focal_points=3, source_size=0.3, source_points=3)


def _dets(ps):
    return [ps.Detector("bf", 0.0, 20.0), ps.Detector("adf", 50.0, 150.0), ps.Detector("comx", 0.0, 40.0, signal="com_x"),
            ps.Detector("comy", 0.0, 40.0, signal="com_y")]


def _polar(ps, per_frame=False):
    return ps.PolarDetector(outer=120.0, step=20.0, n_azimuthal=4, per_frame=per_frame)


@pytest.fixture(scope="module")
def cell(ps):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(64, 4, 2, density=0.1, seed=12)


def _calc(ps, cell, pp=PP, ab=None, **kw):
    calc = ps.MultisliceCalculator(progress=False, aberrations=ab if ab is not None else ps.Aberrations(C10=C10, Cs=CS), **kw)
    calc.setup(cell, aperture=MRAD, voltage_eV=EV, probe_positions=pp)
    return calc


@pytest.fixture(scope="module")
def folded(ps, cell):
    """the host fold of 27 plain scans through the existing API: Aberrations(C10 + delta_g) at positions shifted by d_g -- made once"""
    d, df, w = _coherence(ps).members()
    pat = np.zeros((4, 32, 32))
    det = np.zeros((4, 2, 4))
    pol = np.zeros((4, 6, 4))
    pol_t = np.zeros((4, 2, 6, 4))
    for g in range(len(w)):
        ab = ps.Aberrations(C10=C10 + df[g], Cs=CS)
        pp = [(x + d[g, 0], y + d[g, 1]) for x, y in PP]
        dd = _calc(ps, cell, pp, ab, diffraction=ps.Diffraction(bin=(2, 2)), detectors=_dets(ps)).run_diffraction()
        pat += w[g] * dd.intensity
        det += w[g] * dd.stem.signals
        pol_t += w[g] * _calc(ps, cell, pp, ab, polar=_polar(ps, per_frame=True)).run_polar().signals
    return dict(pat=pat, det=det, pol=pol_t.mean(axis=1), pol_t=pol_t)


@pytest.fixture(scope="module")
def coherent_run(ps, cell):
    return _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2)), detectors=_dets(ps), coherence=_coherence(ps)).run_diffraction()


def test_scan_modes_match_the_fold_of_plain_scans(ps, cell, folded, coherent_run):
    """the bound: waves computed two ways agree to WAVE_TOL = 1e-4 relative L2; intensities inherit at most twice that"""
    c = _coherence(ps)
    dd = coherent_run
    assert dd.intensity.shape == (4, 32, 32) and dd.coherence == c and dd.stem.coherence == c
    st = _calc(ps, cell, detectors=_dets(ps), coherence=c).run_detectors()
    po = _calc(ps, cell, polar=_polar(ps), coherence=c).run_polar()
    pt = _calc(ps, cell, polar=_polar(ps, per_frame=True), coherence=c).run_polar()
    assert st.signals.shape == (4, 2, 4) and po.signals.shape == (4, 6, 4) and pt.signals.shape == (4, 2, 6, 4) and po.coherence == c
    errs = dict(patterns=rel_l2(dd.intensity, folded["pat"]), stem_of_patterns=rel_l2(dd.stem.signals, folded["det"]),
                detectors=rel_l2(st.signals, folded["det"]), polar=rel_l2(po.signals, folded["pol"]),
                polar_per_frame=rel_l2(pt.signals, folded["pol_t"]))
    for k, v in errs.items():
        print(f"G = 27 against the fold of 27 plain scans, {k}: rel-L2 {v:.3e}")
    assert max(errs.values()) <= 2 * WAVE_TOL
    assert np.array_equal(dd.stem.signals, st.signals)                        # the same pass, the same fold
    # the comparison has power: the coherent patterns lie at least ten bounds away from the ensemble's
    plain = _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2))).run_diffraction()
    away = rel_l2(plain.intensity, dd.intensity)
    print(f"the coherent patterns against the ensemble's: rel-L2 {away:.3e}")
    assert away > 10 * 2 * WAVE_TOL


def test_off_is_bitwise_the_run_without(ps, cell):
    a = _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2)), detectors=_dets(ps), coherence=ps.Coherence()).run_diffraction()
    b = _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2)), detectors=_dets(ps)).run_diffraction()
    assert np.array_equal(a.intensity, b.intensity) and np.array_equal(a.stem.signals, b.stem.signals) and a.coherence is None


@pytest.mark.parametrize("probe_batch", [27, 54])
def test_probe_batches_agree(ps, cell, coherent_run, probe_batch):
    calc = _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2)), detectors=_dets(ps), coherence=_coherence(ps), probe_batch=probe_batch + 5)
    assert calc.probe_batch == probe_batch                                    # rounded down to whole positions
    dd = calc.run_diffraction()
    err = np.abs(dd.intensity - coherent_run.intensity).max() / coherent_run.intensity.max()
    serr = np.abs(dd.stem.signals - coherent_run.stem.signals).max() / np.abs(coherent_run.stem.signals).max()
    print(f"probe_batch {probe_batch} against the automatic batch: patterns {err:.3e}, detectors {serr:.3e}")
    assert err <= 1e-6 and serr <= 1e-6


def test_dose_and_camera_do_not_depend_on_the_batch(ps, cell, coherent_run):
    c = _coherence(ps)
    dose = ps.Dose(electrons_per_probe=1e4, seed=7, keep_intensity=True)
    runs = [_calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2), dose=dose), coherence=c, probe_batch=pb).run_diffraction()
            for pb in (27, None)]
    assert runs[0].counts.dtype == np.uint32 and runs[0].counts.shape == (4, 32, 32)
    assert np.array_equal(runs[0].counts, runs[1].counts)
    assert abs(runs[0].counts.sum() / 4e4 - 1.0) < 0.05                        # about N_e electrons per position land on the detector
    # the draw is made from the averaged pattern: the definition's draw of the folded intensity, position by position
    lam = runs[1].intensity * 2 * (1e4 / (2 * runs[1].incident))
    want = ps.poisson_counts(lam, 7, np.arange(4))
    assert int((want != runs[1].counts).sum()) <= 1
    assert rel_l2(runs[1].intensity, coherent_run.intensity) <= 1e-6
    # one frame per frame batch: two msl_dose_add_members per reset, each from frame slot 0 of the ring
    one = _calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2), dose=dose), coherence=c, probe_batch=54, frame_batch=1)
    assert one._engine.frame_batch == 1 and len(one._frame_batches()) == 2
    one = one.run_diffraction()
    err = np.abs(one.intensity - runs[1].intensity).max() / runs[1].intensity.max()
    differ = int((one.counts != runs[1].counts).sum())
    print(f"frame_batch 1 against one batch of 2 frames: intensity {err:.3e}, {differ} of {one.counts.size} counts differ")
    assert err <= 1e-6
    assert int((one.counts != ps.poisson_counts(one.intensity * 2 * (1e4 / (2 * one.incident)), 7, np.arange(4))).sum()) <= 1
    cam = ps.Camera(psf=ps.gaussian_psf(0.7, 2), gain=3.0, offset=20.0, readout_noise=1.5, keep_counts=True)
    frames = [_calc(ps, cell, diffraction=ps.Diffraction(bin=(2, 2), dose=ps.Dose(electrons_per_probe=1e4, seed=7), camera=cam), coherence=c,
                    probe_batch=pb).run_diffraction() for pb in (27, None)]
    assert frames[0].frames.dtype == np.uint16 and np.array_equal(frames[0].frames, frames[1].frames)
    assert np.array_equal(frames[0].counts, runs[0].counts)


def test_source_size_lowers_the_column_and_keeps_the_scan_mean(ps):
    """a column of gold atoms in the middle of the cell, a 10 x 10 raster over the periodic cell (step 0.64 A: the ADF signal is
    band-limited to twice the aperture, 1.35 / A, below the raster's sampling frequency, so the raster mean is the cell mean and a
    shift of the raster does not change it)"""
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(64, 4)
    tr0 = ps.Trajectory(atom_types=np.full(4, 79, dtype=np.int64), positions=np.zeros((1, 4, 3)), velocities=np.zeros((1, 4, 3)),
                        box_matrix=box, timestep=0.005)
    xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr0)
    assert len(xs) == len(ys) == 64 and len(zs) == 4
    Lx, Ly = len(xs) * (xs[1] - xs[0]), len(ys) * (ys[1] - ys[0])                # the period of the grid
    pos = np.zeros((1, 4, 3))
    pos[0, :, 0], pos[0, :, 1] = Lx / 2, Ly / 2
    pos[0, :, 2] = np.clip((np.arange(4) + 0.5) * 0.5, 0.0, np.nextafter(box[2, 2], 0.0))       # one atom in every slice
    tr = ps.Trajectory(atom_types=np.full(4, 79, dtype=np.int64), positions=pos, velocities=np.zeros_like(pos), box_matrix=box, timestep=0.005)
    pp = [(Lx / 2 + (i - 5) * Lx / 10, Ly / 2 + (j - 5) * Ly / 10) for i in range(10) for j in range(10)]
    adf = [ps.Detector("adf", 50.0, 150.0)]
    ab = ps.Aberrations()
    plain = _calc(ps, tr, pp, ab, detectors=adf).run_detectors().signals[:, 0, 0]
    blurred = _calc(ps, tr, pp, ab, detectors=adf, coherence=ps.Coherence(source_size=0.6, source_points=3)).run_detectors().signals[:, 0, 0]
    on = int(np.argmax(plain))
    print(f"ADF on the column: coherent {plain[on]:.6e}, source 0.6 A {blurred[on]:.6e}; scan means {plain.mean():.9e} / {blurred.mean():.9e}")
    assert plain[on] > 2.0 * np.sort(plain)[-2]                               # one position of the raster sits on the column
    assert blurred[on] < 0.9 * plain[on]
    assert abs(blurred.mean() / plain.mean() - 1.0) <= 1e-6

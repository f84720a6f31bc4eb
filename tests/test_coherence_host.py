"""Partial coherence on the host (no device): the member ensemble of coherence.Coherence -- weights, moments, order --, its validation,
the helpers, blur_scan against the quadrature it stands in for, the calculator's refusals and the calls it issues (a RecordingEngine
in the place of _native.Engine), and the three entry points in the header and the symbol table."""
import math
import os
import re

import numpy as np
import pytest

from recording_engine import RecordingEngine

from pyslice_amd import coherence as coh
from pyslice_amd.coherence import Coherence, blur_scan, chromatic_focal_spread, fold_members, fwhm_to_sigma

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- members() -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", [(1, 1), (3, 1), (1, 3), (3, 3), (5, 5), (7, 3)])
def test_members_weights_and_moments(F, S):
    D, sg = 40.0, 0.3
    c = Coherence(focal_spread=D if F > 1 else 0.0, focal_points=F, source_size=sg if S > 1 else 0.0, source_points=S)
    d, df, w = c.members()
    G = F * S * S
    assert c.n_members == G and d.shape == (G, 2) and df.shape == (G,) and w.shape == (G,)
    assert d.dtype == df.dtype == w.dtype == np.float64
    assert abs(w.sum() - 1.0) <= 1e-15
    assert (w > 0).all()
    if F > 1:
        assert abs((w * df ** 2).sum() - D * D) <= 1e-12 * D * D
    else:
        assert (df == 0).all()
    for ax in (0, 1):
        if S > 1:
            assert abs((w * d[:, ax] ** 2).sum() - sg * sg) <= 1e-12 * sg * sg
        else:
            assert (d[:, ax] == 0).all()
    # odd moments vanish (against the scale of the matching even moment)
    assert abs((w * df).sum()) <= 1e-12 * D and abs((w * df ** 3).sum()) <= 1e-12 * D ** 3
    for ax in (0, 1):
        assert abs((w * d[:, ax]).sum()) <= 1e-12 * sg and abs((w * d[:, ax] ** 3).sum()) <= 1e-12 * sg ** 3
    assert abs((w * d[:, 0] * d[:, 1]).sum()) <= 1e-12 * sg * sg


def test_members_order_and_product_weights():
    c = Coherence(focal_spread=50.0, focal_points=3, source_size=0.5, source_points=5)
    d, df, w = c.members()
    fd, fw = c.focal_nodes()
    sd, sw = c.source_nodes()
    F, S = 3, 5
    for f in range(F):
        for ix in range(S):
            for iy in range(S):
                g = (f * S + ix) * S + iy
                assert df[g] == fd[f] and d[g, 0] == sd[ix] and d[g, 1] == sd[iy]
                assert w[g] == fw[f] * (sw[ix] * sw[iy])


def test_focal_nodes_are_imagings():
    from pyslice_amd import Imaging
    for n, D in ((3, 40.0), (5, 61.5), (1, 0.0)):
        a = Coherence(focal_spread=D, focal_points=n).focal_nodes()
        b = Imaging(focal_spread=D, focal_points=n).nodes()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_default_is_off():
    c = Coherence()
    assert c.is_off and c.n_members == 1
    d, df, w = c.members()
    assert np.array_equal(d, [[0.0, 0.0]]) and np.array_equal(df, [0.0]) and np.array_equal(w, [1.0])
    assert Coherence(focal_spread=30.0).is_off                 # a width without points is one node


@pytest.mark.parametrize("kw", [
    dict(focal_spread=10.0, focal_points=2), dict(source_size=0.3, source_points=4), dict(focal_points=0), dict(source_points=-1),
    dict(focal_spread=-1.0), dict(source_size=-0.1), dict(focal_points=3), dict(source_points=3), dict(focal_spread=float("nan")),
    dict(source_size=float("inf")), dict(focal_spread=10.0, focal_points=3.0), dict(focal_points=True), dict(focal_spread="x"),
    dict(focal_spread=10.0, focal_points=7, source_size=0.3, source_points=5),          # 175 members
    dict(source_size=0.3, source_points=13),                                            # 169 members
])
def test_validation(kw):
    with pytest.raises(ValueError, match="Coherence"):
        Coherence(**kw)


def test_largest_ensemble_fits():
    assert Coherence(focal_spread=10.0, focal_points=5, source_size=0.3, source_points=5).n_members == 125
    assert coh.MEMBERS_MAX == 128


def test_frozen():
    with pytest.raises(Exception):
        Coherence().focal_spread = 3.0


def test_helpers():
    # Cc = 1.2 mm, dE = 0.3 eV rms at 200 kV: 1.2e7 * 1.5e-6 * (1 + 0.391389...) / (1 + 0.195694...) = 20.9459... Angstrom
    want = 1.2e7 * (0.3 / 200e3) * (1 + 200.0 / 511.0) / (1 + 100.0 / 511.0)
    assert abs(chromatic_focal_spread(1.2e7, 0.3, 200e3) - want) <= 1e-12 * want
    assert abs(want - 20.9459) < 1e-3
    assert abs(fwhm_to_sigma(2.0 * math.sqrt(2.0 * math.log(2.0))) - 1.0) <= 1e-15
    assert abs(fwhm_to_sigma(1.0) - 0.42466090014400953) <= 1e-15


def test_fold_members():
    rng = np.random.default_rng(0)
    v = rng.random((6, 2, 3))
    w = np.array([0.2, 0.5, 0.3])
    got = fold_members(v, w)
    want = np.zeros((2, 2, 3))
    for q in range(2):
        for g in range(3):
            want[q] = want[q] + w[g] * v[q * 3 + g]
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        fold_members(v[:5], w)


# ---- blur_scan -------------------------------------------------------------------------------------------
def _signal():
    """a smooth periodic signal on a 3.2 x 3.2 Angstrom cell by its Fourier content: (hx, hy, amplitude, phase)"""
    return 2.0, [(1, 0, 0.7, 0.3), (0, 1, 0.5, -1.1), (1, 1, 0.3, 0.8), (2, -1, 0.2, 2.0), (0, 2, 0.15, -0.4), (3, 2, 0.05, 1.3)]


def _evaluate(x, y, L=3.2):
    mean, terms = _signal()
    out = np.full(np.broadcast(x, y).shape, mean)
    for hx, hy, a, ph in terms:
        out = out + a * np.cos(2 * np.pi * (hx * x + hy * y) / L + ph)
    return out


def test_blur_scan_preserves_sum_and_identity():
    rng = np.random.default_rng(1)
    v = rng.random((16, 12, 3))
    assert np.array_equal(blur_scan(v, (0.2, 0.3), 0.0), v)
    for periodic in (True,):
        b = blur_scan(v, (0.2, 0.3), 0.4, periodic=periodic)
        assert b.shape == v.shape
        assert np.all(np.abs(b.sum(axis=(0, 1)) - v.sum(axis=(0, 1))) <= 1e-12 * v.sum(axis=(0, 1)))
    flat = np.full((9, 7), 3.5)
    assert np.allclose(blur_scan(flat, (0.2, 0.2), 0.5, periodic=False), 3.5, rtol=1e-13, atol=0)
    assert blur_scan(rng.random((9, 7)), (0.2, 0.2), 0.5, periodic=False).shape == (9, 7)


def test_blur_scan_is_the_source_quadrature():
    """16 x 16 periodic raster, step 0.2, sigma_s = 0.4: blur_scan of the sampled signal against the S = 5 quadrature average of the
    analytic signal at the member positions.  blur_scan is exact for the band-limited signal (every term below the raster's Nyquist
    index 8), so the difference is the quadrature's error: per Fourier term |a| * |prod_axis sum_i w_i cos(2 pi h d_i / L) -
    exp(-2 pi^2 sigma^2 q^2)| (the sine parts cancel in the symmetric rule)."""
    L, n, sigma = 3.2, 16, 0.4
    step = L / n
    x = (np.arange(n) * step)[:, None]
    y = (np.arange(n) * step)[None, :]
    d, _, w = Coherence(source_size=sigma, source_points=5).members()
    quad = np.zeros((n, n))
    for g in range(len(w)):
        quad += w[g] * _evaluate(x + d[g, 0], y + d[g, 1], L)
    got = blur_scan(_evaluate(x, y, L), (step, step), sigma, periodic=True)
    nodes, nw = Coherence(source_size=sigma, source_points=5).source_nodes()
    bound = 0.0
    for hx, hy, a, _ in _signal()[1]:
        q_rule = (nw * np.cos(2 * np.pi * hx * nodes / L)).sum() * (nw * np.cos(2 * np.pi * hy * nodes / L)).sum()
        exact = math.exp(-2 * math.pi ** 2 * sigma ** 2 * (hx * hx + hy * hy) / L ** 2)
        bound += abs(a) * abs(q_rule - exact)
    err = np.abs(got - quad).max()
    print(f"blur_scan vs S=5 quadrature: max |diff| {err:.3e}, quadrature error bound {bound:.3e}")
    assert bound < 0.05                                        # (the rule is a fair stand-in at this sigma: the bound says how fair)
    assert err <= bound + 1e-12


def test_source_blurred_needs_a_raster():
    from pyslice_amd import Detector, STEMData
    det = [Detector("adf", 60.0, 200.0)]
    xs, ys = np.arange(4) * 0.5, np.arange(3) * 0.7
    pp = [(float(a), float(b)) for a in xs for b in ys]
    sig = np.random.default_rng(2).random((12, 2, 1))
    s = STEMData(signals=sig, detectors=det, probe_positions=pp, time=np.arange(2.0), kxs=None, kys=None, probe=None)
    b = s.source_blurred(0.3)
    want = blur_scan(sig.reshape(4, 3, 2, 1), (0.5, 0.7), 0.3).reshape(12, 2, 1)
    assert np.array_equal(b.signals, want) and b.signals.shape == sig.shape
    # any order of the positions
    perm = np.random.default_rng(3).permutation(12)
    s2 = STEMData(signals=sig[perm], detectors=det, probe_positions=[pp[i] for i in perm], time=np.arange(2.0), kxs=None, kys=None, probe=None)
    assert np.array_equal(s2.source_blurred(0.3).signals, want[perm])
    bad = STEMData(signals=sig[:11], detectors=det, probe_positions=pp[:11], time=np.arange(2.0), kxs=None, kys=None, probe=None)
    with pytest.raises(ValueError, match=r"^source_blurred: .*raster of their coordinates$"):
        bad.source_blurred(0.3)
    with pytest.raises(ValueError, match=r"^blur_scan: sigma must not be negative"):
        s.source_blurred(-0.3)


def test_polar_source_blurred():
    from pyslice_amd import PolarData, PolarDetector
    pol = PolarDetector(outer=40.0, step=10.0)
    pp = [(float(a), float(b)) for a in (0.0, 0.4, 0.8) for b in (0.0, 0.5)]
    sig = np.random.default_rng(4).random((6, pol.n_rings, 1))
    data = PolarData(signals=sig, polar=pol, counts=np.ones((pol.n_rings, 1)), edges=pol.edges, probe_positions=pp, time=np.arange(1.0),
                     kxs=None, kys=None, probe=None)
    got = data.source_blurred(0.25).signals
    assert np.array_equal(got, blur_scan(sig.reshape(3, 2, pol.n_rings, 1), (0.4, 0.5), 0.25).reshape(sig.shape))
    with pytest.raises(ValueError, match="raster"):
        PolarData(signals=sig[:5], polar=pol, counts=np.ones((pol.n_rings, 1)), edges=pol.edges, probe_positions=pp[:5],
                  time=np.arange(1.0), kxs=None, kys=None, probe=None).source_blurred(0.25)


# ---- the calculator: refusals ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traj():
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(64, 6, 2, density=0.05, seed=4)


def _calc(**kw):
    from pyslice_amd.calculators import MultisliceCalculator
    return MultisliceCalculator(progress=False, **kw)


ON = dict(focal_spread=40.0, focal_points=3)


def _refusals():
    from pyslice_amd import Detector, Diffraction, Imaging, Ionization, PolarDetector, Precession, Spectroscopy
    from pyslice_amd.prism import Prism
    det = [Detector("adf", 60.0, 200.0)]
    return [
        ("split", dict(diffraction=Diffraction(split=True))),
        ("thickness", dict(detectors=det, thickness=[1, 3])),
        ("layers", dict(layers=[1])),
        ("prism", dict(detectors=det, prism=Prism(1))),
        ("precession", dict(detectors=det, precession=Precession(10.0, 4))),
        ("tds", dict(detectors=det, tds=True)),
        ("ionization", dict(ionization=[Ionization("Si", 0.3, 1.0)])),
        ("spectroscopy", dict(spectroscopy=Spectroscopy(detectors=det))),
        ("imaging", dict(imaging=Imaging())),
        ("run", dict()),
        ("cache", dict(cache=True)),
        ("stream_tile", dict(stream_tile=2)),
    ]


@pytest.mark.parametrize("name,kw", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_name_coherence(name, kw):
    with pytest.raises(NotImplementedError, match=r"coherence: .* is not built"):
        _calc(coherence=Coherence(**ON), **kw)
    _calc(coherence=Coherence(), **{k: v for k, v in kw.items() if k not in ("cache",)})      # off: nothing to refuse


def test_run_methods_refused():
    from pyslice_amd import Detector
    calc = _calc(coherence=Coherence(**ON), detectors=[Detector("adf", 60.0, 200.0)])
    with pytest.raises(NotImplementedError, match=r"coherence: run\(\) is not built"):
        calc.run()
    with pytest.raises(NotImplementedError, match=r"coherence: run_streaming_tacaw\(\) is not built"):
        calc.run_streaming_tacaw()


def test_type_checked():
    with pytest.raises(ValueError, match="coherence"):
        _calc(coherence=3)


def test_setup_refusals_before_device_work(traj, monkeypatch):
    from pyslice_amd import Detector, _native, distributed

    def no_engine(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(_native, "Engine", no_engine)
    det = [Detector("adf", 60.0, 200.0)]
    with pytest.raises(ValueError, match="coherence needs a convergent probe"):
        _calc(coherence=Coherence(**ON), detectors=det).setup(traj, aperture=0.0, voltage_eV=100e3)
    with pytest.raises(ValueError, match=r"coherence: probe_batch=2 is below the G = 3"):
        _calc(coherence=Coherence(**ON), detectors=det, probe_batch=2).setup(traj, aperture=30.0, voltage_eV=100e3)
    monkeypatch.setattr(distributed, "rank_world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"coherence: a run over several ranks is not built"):
        _calc(coherence=Coherence(**ON), detectors=det).setup(traj, aperture=30.0, voltage_eV=100e3)


# ---- the calculator: the calls it issues -----------------------------------------------------------------
class MemberEngine(RecordingEngine):
    """RecordingEngine that also answers the member reductions, the polar pass and the dose draw with arrays of the right shape"""
    n_bins = 0

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)

        def wrapped(*a, **k):
            out = call(*a, **k)
            mx, my = self.wx // k.get("bin", (1, 1))[0], self.wy // k.get("bin", (1, 1))[1]
            if name == "diffract_members":
                return np.ones((k["B"] // len(a[0]), mx, my)) * a[2]
            if name == "set_polar":
                self.n_bins = a[1]
            if name == "polar_detect":
                return np.ones((k["B"], a[1], self.n_bins))
            if name == "dose_reset":
                self._dose = (a[0],) + tuple(a[1])
            if name == "dose_counts":
                return np.zeros((k["B"],) + self._dose[1:], dtype=np.uint32), None
            return out
        return wrapped


@pytest.fixture
def engines(monkeypatch):
    from pyslice_amd import _native
    made = []

    def make(*a, **k):
        made.append(MemberEngine(*a, **k))
        return made[-1]
    monkeypatch.setattr(_native, "Engine", make)
    monkeypatch.setattr("pyslice_amd.calculators._free_device_bytes", lambda dev: None)
    return made


PP = [(1.0, 1.0), (2.0, 3.0), (2.5, 0.5), (3.0, 3.5), (0.5, 2.0)]


def _names(eng):
    return [c[0] for c in eng.calls]


def test_off_takes_todays_path(traj, engines):
    from pyslice_amd import Diffraction
    for kw in (dict(coherence=Coherence()), dict()):
        calc = _calc(diffraction=Diffraction(bin=(2, 2)), **kw)
        calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
        out = calc.run_diffraction()
        assert calc.coherence_members is None and out.coherence is None
    a, b = engines
    assert a.created == b.created and _names(a) == _names(b)
    assert "set_probes" in _names(a) and not any("member" in n for n in _names(a))


def test_member_calls(traj, engines):
    from pyslice_amd import Detector, Diffraction
    c = Coherence(**ON)
    calc = _calc(diffraction=Diffraction(bin=(2, 2)), detectors=[Detector("bf", 0.0, 20.0)], coherence=c, probe_batch=7)
    calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    eng = engines[-1]
    assert eng.n_probes == 6 and calc.probe_batch == 6           # 7 rounded down to a multiple of G = 3
    d, df, w = calc.coherence_members
    assert np.array_equal(w, c.members()[2])
    out = calc.run_diffraction()
    assert out.coherence is c and out.stem.coherence is c
    assert out.intensity.shape == (5, 32, 32) and out.stem.signals.shape == (5, 2, 1)
    assert "set_probes" not in _names(eng) and "diffract" not in _names(eng)
    sets = [c_ for c_ in eng.calls if c_[0] == "set_probe_members"]
    folds = [c_ for c_ in eng.calls if c_[0] == "diffract_members"]
    pos = np.asarray(PP)
    # 5 positions at 2 per batch: (0, 1), (2, 3), (4, 4 again: the short batch is padded by a whole position)
    want_q = [[0, 1], [2, 3], [4, 4]]
    assert len(sets) == len(want_q) * len(calc._frame_batches())
    for (name, a, k), q in zip(sets, want_q * len(calc._frame_batches())):
        assert a[0] == 30.0
        want_xy = (pos[q][:, None, :] + d[None, :, :]).reshape(-1, 2)
        assert np.array_equal(a[1], want_xy) and a[1].shape == (6, 2)
        assert np.array_equal(a[2], np.tile(df, 2))
    for (name, a, k), real in zip(folds, [2, 2, 1] * len(calc._frame_batches())):
        assert np.array_equal(a[0], w) and k["B"] == real * 3 and k["B"] % 3 == 0 and k["bin"] == (2, 2)
    dets = [c_ for c_ in eng.calls if c_[0] == "detect"]
    assert [k["B"] for _, _, k in dets] == [6, 6, 3] * len(calc._frame_batches())


def test_member_calls_dose_and_polar(traj, engines):
    from pyslice_amd import Diffraction, Dose, PolarDetector
    c = Coherence(source_size=0.3, source_points=3)             # G = 9
    calc = _calc(diffraction=Diffraction(bin=(1, 1), dose=Dose(electrons_per_probe=100.0, seed=3)), coherence=c, probe_batch=20)
    calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    eng = engines[-1]
    assert eng.n_probes == 18
    out = calc.run_diffraction()
    assert out.counts.shape == (5, 64, 64) and out.coherence is c
    names = _names(eng)
    assert "dose_add" not in names and "set_probes" not in names
    adds = [(a, k) for n, a, k in eng.calls if n == "dose_add_members"]
    assert [k["B"] for a, k in adds] == [18, 18, 9] and all(len(a[0]) == 9 for a, k in adds)
    assert [a[0] for n, a, k in eng.calls if n == "dose_reset"] == [2, 2, 1]         # sized for POSITIONS
    draws = [k for n, a, k in eng.calls if n == "dose_counts"]
    assert [(k["probe0"], k["B"]) for k in draws] == [(0, 2), (2, 2), (4, 1)]         # keyed by the position's index in the scan

    calc = _calc(polar=PolarDetector(outer=40.0, step=10.0, per_frame=True), coherence=c)
    calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    eng = engines[-1]
    assert eng.n_probes == 45                                    # all 5 positions x 9 members: below the automatic 256 // 9 * 9
    out = calc.run_polar()
    assert out.signals.shape == (5, 2, 4, 1) and out.coherence is c
    assert np.allclose(out.signals, 1.0, rtol=1e-14)             # the weights sum to 1
    assert "set_probe_members" in _names(eng) and "set_probes" not in _names(eng)


def test_auto_batch_is_whole_positions(traj, engines):
    from pyslice_amd import Detector
    c = Coherence(focal_spread=40.0, focal_points=3, source_size=0.3, source_points=3)     # G = 27
    pp = [(0.1 * i, 0.2 * j) for i in range(6) for j in range(5)]                         # 30 positions = 810 waves
    calc = _calc(detectors=[Detector("adf", 60.0, 200.0)], coherence=c)
    calc.setup(traj, aperture=30.0, voltage_eV=100e3, probe_positions=pp)
    assert engines[-1].n_probes == 256 // 27 * 27 == 243
    out = calc.run_detectors()
    assert out.signals.shape == (30, 2, 1)
    sets = [a for n, a, k in engines[-1].calls if n == "set_probe_members"]
    assert all(a[1].shape == (243, 2) and a[2].shape == (243,) for a in sets)


# ---- the ABI ---------------------------------------------------------------------------------------------
def test_header_and_symbol_table():
    from pyslice_amd import _native
    text = open(os.path.join(REPO, "include", "mslice.h")).read()
    assert re.search(r"#define\s+MSL_ABI_VERSION\s+3\b", text) and _native.ABI_VERSION == 3
    assert re.search(r"#define\s+MSL_MEMBERS_MAX\s+128\b", text) and _native.MEMBERS_MAX == 128 == coh.MEMBERS_MAX
    for fn in ("msl_set_probe_members", "msl_diffract_members", "msl_dose_add_members"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(msl_handle\*", text), fn
        assert fn in _native.EXPORTS

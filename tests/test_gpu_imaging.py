"""HRTEM images on the MI355X: msl_image_add on caller-held spectra against float64 NumPy, the refusals of the three entry points,
known answers through run_images() (vacuum, the identity lens, defocus as propagation, the focal spread) and run_images() against
the oracle with its own frame / probe batching."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

LAM = 0.037


@pytest.fixture(scope="module")
def ps():
    import pyslice_amd
    from pyslice_amd import _native
    _native.load()
    return pyslice_amd


def _prime_factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    if n > 1:
        out.append(n)
    return out or [1]


def tol_fft(shape):
    """the rule of test_fft2_matches_numpy: 3e-6 when both lengths have prime factors <= 13, 1e-5 otherwise (Bluestein lines)"""
    return 3e-6 if all(max(_prime_factors(n)) <= 13 for n in shape) else 1e-5


def image_tol(shape):
    """an amplitude error e is at most 2e in |psi|^2; the lens phase costs one fp32 sincospif of a reduced turn; float64 sums"""
    return 2 * tol_fft(shape) + 2e-6


# ------------------------------------------------------------------ 1. the kernel pass on caller-held spectra
DX, DY = 0.1, 0.12
B, T = 3, 4
SHAPES = [(32, 32),        # 16-byte path
          (45, 63),        # both lengths odd: the shift and 8-byte accesses
          (96, 80),        # generic lines
          (256, 144),      # ny % 32 = 16
          (135, 256),      # direct mixed radix x power of two
          (1024, 64),      # radix-32 columns
          (167, 64),       # a convolution / Bluestein line
          (36, 30)]        # ny even, ny / 2 odd: an even column shifts to an odd one (8-byte loads, 16-byte sums)


def _lenses(nx, ny):
    """(name, Imaging): none; aperture only; defocus + Cs with |chi| > 300 rad inside the aperture + an m > 0 term with an angle"""
    from pyslice_amd import Aberrations, Imaging
    k_ap = 0.613 * min(0.5 / DX, 0.5 / DY)                    # inside Nyquist of both axes
    mrad = k_ap * LAM * 1e3
    strong = Aberrations(C10=-350.0, Cs=1.0e6, C12=80.0, phi12=0.6, C23=4000.0, phi23=-0.9)
    return [("none", Imaging()), ("aperture", Imaging(aperture_mrad=mrad)), ("strong", Imaging(aberrations=strong, aperture_mrad=mrad))]


@pytest.fixture(scope="module")
def kernel_inputs():
    """per shape: the white spectra (B, T, nx*ny) complex64 at mixed scales and, per lens, the float64 NumPy |psi|^2 of every
    (b, t) -- computed once, shared by the ld cases and the chunking case"""
    cache = {}

    def get(shape):
        if shape not in cache:
            nx, ny = shape
            rng = np.random.default_rng(nx * 10007 + ny)
            W = (rng.standard_normal((B, T, nx * ny)) + 1j * rng.standard_normal((B, T, nx * ny))).astype(np.complex64)
            W *= rng.choice([1e-3, 1.0, 30.0], size=(B, T, 1)).astype(np.float32)
            kx, ky = np.fft.fftfreq(nx, DX)[:, None], np.fft.fftfreq(ny, DY)[None, :]
            spec = np.fft.ifftshift(W.astype(np.complex128).reshape(B, T, nx, ny), axes=(-2, -1))
            per_lens = {}
            for name, im in _lenses(nx, ny):
                H = im.transfer(kx, ky, LAM)
                if name == "strong":
                    inside = np.abs(H) > 0
                    assert np.abs(im.aberrations.chi(kx, ky, LAM))[inside].max() > 300.0
                per_lens[name] = np.abs(np.fft.ifft2(spec * H, axes=(-2, -1))) ** 2
            cache[shape] = (W, per_lens)
        return cache[shape]
    return get


def _device_source(W, ld_pad):
    import torch
    K = W.shape[-1]
    host = np.full((B, T, K + ld_pad), np.nan + 1j * np.nan, dtype=np.complex64)      # pad pixels must never be read
    host[:, :, :K] = W
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return d


def _kernel_engine(shape, frame_batch):
    from pyslice_amd import _native
    return _native.Engine(shape[0], shape[1], 1, DX, DY, 1.0, LAM, 0.0, n_probes=B, n_frames=0, device=0, frame_batch=frame_batch)


RANGES = [(0, 1), (0, min(3, T)), (0, T), (1, 2), (T - 1, 1)]


@pytest.mark.parametrize("ld_pad", [0, 3, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_image_pass_matches_numpy(ps, kernel_inputs, shape, ld_pad):
    """msl_image_add on caller-held device memory: every image to 2 tol_fft + 2e-6 rel-L2 of float64 NumPy on the same complex64
    values; untouched accumulator images stay zero; repeats and split frame ranges are bitwise equal"""
    nx, ny = shape
    W, want_all = kernel_inputs(shape)
    dW = _device_source(W, ld_pad)
    eng = _kernel_engine(shape, T)                              # the work buffer holds B * T images: one chunk
    tol = image_tol(shape)
    try:
        src = (dW.data_ptr(), B, T, nx * ny + ld_pad)
        first, stride, n_img, weight = 2, 3, 2 + 3 * B, 0.37
        for name, im in _lenses(nx, ny):
            kw = dict(polar=None if name != "strong" else im.polar(), aperture_k=im.aperture_k(LAM), weight=weight, first=first, stride=stride, src=src)
            for t0, count in RANGES:
                eng.image_reset(n_img)
                eng.image_add(t0, count, **kw)
                got = eng.image_download(0, n_img)
                assert got.shape == (n_img, nx, ny) and got.dtype == np.float64
                want = weight * want_all[name][:, t0:t0 + count].sum(axis=1)
                errs = [rel_l2(got[first + b * stride], want[b]) for b in range(B)]
                print(f"shape {shape} ld+{ld_pad} lens {name} frames [{t0},{t0 + count}): max rel-L2 {max(errs):.3e} (bound {tol:.1e})")
                assert max(errs) <= tol, (name, t0, count, errs)
                others = np.delete(got, [first + b * stride for b in range(B)], axis=0)
                assert not others.any()                         # only first + b * stride were written
                eng.image_reset(n_img)
                eng.image_add(t0, count, **kw)
                assert np.array_equal(eng.image_download(0, n_img), got)          # no atomics: bitwise reproducible
            # [0, T) in one call == [0, s) then [s, T), bitwise; count = None is the rest of the frames
            eng.image_reset(n_img)
            eng.image_add(0, None, **kw)
            whole = eng.image_download(first, 1 + (B - 1) * stride)
            for s in (1, 3):
                eng.image_reset(n_img)
                eng.image_add(0, s, **kw)
                eng.image_add(s, T - s, **kw)
                assert np.array_equal(eng.image_download(first, 1 + (B - 1) * stride), whole), (name, s)
    finally:
        eng.close()


@pytest.mark.parametrize("shape", [(45, 63), (96, 80), (256, 144)])
def test_image_pass_chunks_when_the_work_buffer_is_smaller(ps, kernel_inputs, shape):
    """B * count = 12 images through a work buffer of B = 3: the call walks the frames in chunks and gives bitwise the images of the
    one-chunk engine"""
    nx, ny = shape
    W, want_all = kernel_inputs(shape)
    dW = _device_source(W, 3)
    im = _lenses(nx, ny)[2][1]
    kw = dict(polar=im.polar(), aperture_k=im.aperture_k(LAM), weight=1.0, first=0, stride=1, src=(dW.data_ptr(), B, T, nx * ny + 3))
    got = []
    for frame_batch in (T, 1):
        eng = _kernel_engine(shape, frame_batch)
        try:
            eng.image_reset(B)
            eng.image_add(0, T, **kw)
            got.append(eng.image_download(0, B))
        finally:
            eng.close()
    want = want_all["strong"].sum(axis=1)
    errs = [rel_l2(got[1][b], want[b]) for b in range(B)]
    print(f"shape {shape} chunked: max rel-L2 {max(errs):.3e}")
    assert max(errs) <= image_tol(shape)
    assert np.array_equal(got[0], got[1])


# ------------------------------------------------------------------ 2. refusals of the three entry points
def test_image_refusals(ps):
    import torch
    from pyslice_amd import _native
    nx, ny, K = 6, 8, 48
    eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 1.0, LAM, 0.0, n_probes=2, n_frames=0, device=0)
    try:
        d = torch.zeros((2, 3, 50), dtype=torch.complex64, device="cuda")
        p = d.data_ptr()
        ok = dict(src=(p, 2, 3, 50))
        with pytest.raises(ValueError):
            eng.image_add(0, 1, **ok)                            # before any reset: no accumulator image
        for n in (0, -1):
            with pytest.raises(ValueError):
                eng.image_reset(n)
        eng.image_reset(4)
        eng.image_add(0, 3, first=1, stride=2, **ok)
        assert eng.image_download(0, 4).shape == (4, nx, ny)
        nan, inf = float("nan"), float("inf")
        bad_polar = np.zeros((14, 2))
        bad_polar[3, 1] = inf
        for kw in (dict(src=(p, 2, 3, 47)),                                    # ld < nx * ny
                   dict(t0=2, count=2, **ok), dict(t0=-1, count=1, **ok), dict(t0=3, count=1, **ok),      # frames outside [0, T)
                   dict(t0=0, count=0, **ok), dict(t0=0, count=-2, **ok),       # count < 1
                   dict(polar=bad_polar, **ok), dict(weight=nan, **ok), dict(weight=inf, **ok), dict(aperture_k=nan, **ok),
                   dict(aperture_k=-inf, **ok),
                   dict(first=3, stride=1, **ok), dict(first=0, stride=4, **ok), dict(first=4, **ok), dict(first=-1, **ok),   # beyond the reset
                   dict(stride=-1, first=3, **ok),                              # stride < 0
                   dict(stride=0, **ok),                                        # two probes into one image
                   dict(src=(p, 0, 3, 50)), dict(src=(p, 2, 0, 50)),
                   dict(src=(p, 3, 2, 50))):                                    # B above the images of the work buffer
            with pytest.raises(ValueError):
                eng.image_add(**({"t0": 0, "count": 1} | kw))
        with pytest.raises(RuntimeError):
            eng.image_add(0, 1)                                  # d_src == NULL and no result ring: MSL_ERR_STATE
        for first, n in ((0, 5), (4, 1), (-1, 1), (0, 0)):
            with pytest.raises(ValueError):
                eng.image_download(first, n)
        rc = eng._lib.msl_image_download(eng._h, 0, 1, None)
        assert rc == _native.MSL_ERR_INVALID
        eng.image_reset(2)                                       # a smaller reset shrinks what may be addressed
        with pytest.raises(ValueError):
            eng.image_download(0, 4)
        with pytest.raises(ValueError):
            eng.image_add(0, 1, first=1, stride=2, **ok)
    finally:
        eng.close()
    # a handle with a k-window or bins stores no full spectrum
    for kw in (dict(window=(4, 4)), dict(k_bin=(2, 2))):
        eng = _native.Engine(nx, ny, 1, 0.1, 0.1, 1.0, LAM, 0.0, n_probes=2, n_frames=1, device=0, **kw)
        try:
            with pytest.raises(ValueError):
                eng.image_reset(2)
            with pytest.raises(ValueError):
                eng.image_add(0, 1)
        finally:
            eng.close()


# ------------------------------------------------------------------ 3. known answers through run_images()
def _stack(nz, d, n_frames, n=64, n_atoms=40, seed=5, z_top=None, amplitude=0.05):
    """gold atoms in a box of n x n pixels x nz slices of EXACTLY d Angstrom (d < 0.5: gridFromTrajectory then gives nz slices),
    all below z_top"""
    from pyslice_amd.trajectory import Trajectory
    lx = (n - 0.5) * 0.1
    box = np.diag([lx, lx, nz * d])
    rng = np.random.default_rng(seed)
    z_top = nz * d if z_top is None else z_top
    pos0 = rng.random((n_atoms, 3)) * [lx, lx, z_top - 0.2] + [0.0, 0.0, 0.1]
    positions = np.stack([pos0 + np.concatenate([amplitude * rng.standard_normal((n_atoms, 2)), np.zeros((n_atoms, 1))], axis=1)
                          for _ in range(n_frames)])
    return Trajectory(atom_types=np.full(n_atoms, 79, dtype=np.int64), positions=positions, velocities=np.zeros_like(positions),
                      box_matrix=box, timestep=0.005)


def _images(ps, tr, imaging, pp=None, **kw):
    calc = ps.MultisliceCalculator(progress=False, imaging=imaging, **kw)
    calc.setup(tr, aperture=0.0, voltage_eV=100e3, probe_positions=pp)
    return calc, calc.run_images()


@pytest.mark.parametrize("spread", [False, True])
def test_vacuum_images_are_one(ps, spread):
    """no atoms in any slice (two far outside the slices keep the species list alive): every image is 1 for any lens whose
    aperture contains k = 0"""
    from pyslice_amd import Aberrations, Imaging
    from pyslice_amd.trajectory import Trajectory
    n, nz = 48, 4
    box = np.diag([(n - 0.5) * 0.1, (n + 32 - 0.5) * 0.1, (nz - 0.5) * 0.5])
    pos = np.tile(np.array([[1.0, 1.0, 50.0], [2.0, 2.0, 60.0]]), (2, 1, 1))           # z far above the last slice: in no slice
    tr = Trajectory(atom_types=np.array([6, 6]), positions=pos, velocities=np.zeros_like(pos), box_matrix=box, timestep=0.005)
    im = Imaging(aberrations=Aberrations(Cs=1.2e7, C10=-500.0, C12=40.0, phi12=0.3), aperture_mrad=15.0, defocus_series=(-200.0, 0.0, 300.0),
                 **(dict(focal_spread=40.0, focal_points=5) if spread else {}))
    calc, data = _images(ps, tr, im, frame_batch=2)
    assert data.intensity.shape == (1, 1, 3, 48, 80)
    err = np.abs(data.intensity - 1.0).max()
    rl2 = max(rel_l2(data.image(f), np.ones((48, 80))) for f in range(3))
    print(f"vacuum, focal spread {spread}: max |I - 1| {err:.3e}, max rel-L2 {rl2:.3e}")
    assert rl2 <= image_tol((48, 80))


@pytest.fixture(scope="module")
def defocus_case(ps):
    """an 8-slice gold stack A, and B = A with one empty slice appended (same slice thickness d, the atoms below 7.4 d fall into the
    same slices of both); exit waves of both from the device's own msl_propagate, and of B from the oracle"""
    from oracle import multislice_oracle as orc
    from pyslice_amd import _native
    from pyslice_amd.potentials import slice_edges
    d, nz = 0.49, 8
    A = _stack(nz, d, 1, z_top=7.4 * d, amplitude=0.0)
    Bt = _stack(nz + 1, d, 1, z_top=7.4 * d, amplitude=0.0)
    assert np.array_equal(A.positions, Bt.positions)
    exits = {}
    for name, tr in (("A", A), ("B", Bt)):
        xs, ys, zs, lx, ly, lz = ps.gridFromTrajectory(tr)
        assert (len(xs), len(ys), len(zs)) == (64, 64, nz + (name == "B")) and abs((zs[1] - zs[0]) - d) < 1e-12
        eng = _native.Engine(64, 64, len(zs), xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0], ps.wavelength(100e3),
                             orc.interaction_sigma(100e3), n_probes=1, n_frames=0)
        eng.set_kirkland(ps.loadKirkland())
        eng.set_slices(*slice_edges(zs))
        eng.set_probes(0.0, np.zeros((1, 2)))
        eng.build_potential(tr.positions[0], tr.atom_types.astype(np.int32))
        eng.propagate()
        exits[name] = np.abs(eng.exit_waves()[0].astype(np.complex128)) ** 2
        eng.close()
    wf = orc.run_frames(Bt.box_matrix, Bt.positions, Bt.atom_types, 0.0, 100e3)["wavefunction_data"][0, 0, :, :, 0]
    oracle_B = np.abs(np.fft.ifft2(np.fft.ifftshift(wf))) ** 2
    return d, A, exits, oracle_B


def test_identity_lens_gives_the_exit_intensity(ps, defocus_case):
    """no aberrations, no aperture: the image is |MSL_BUF_EXIT|^2 of msl_propagate on the same potential, to 4 tol_fft + 2e-6 (the
    exit FFT and the image's inverse FFT, each at most 2 tol_fft in |psi|^2)"""
    from pyslice_amd import Imaging
    d, A, exits, _ = defocus_case
    calc, data = _images(ps, A, Imaging())
    err = rel_l2(data.image(), exits["A"])
    print(f"identity lens: rel-L2 {err:.3e} (bound {4 * tol_fft((64, 64)) + 2e-6:.1e})")
    assert err <= 4 * tol_fft((64, 64)) + 2e-6


def test_defocus_is_propagation(ps, defocus_case):
    """defocus = +dz (the slice spacing), no aperture: the image of the nz-slice stack is the exit intensity of the stack with one
    empty slice appended -- against the oracle and against the device's own msl_propagate, rel-L2 <= 2e-4.  defocus = -dz is NOT:
    its error must exceed the bound divided by the contrast std / mean of the image (i.e. measured against the part of the image
    that carries structure, it misses by more than the bound)."""
    from pyslice_amd import Imaging
    d, A, exits, oracle_B = defocus_case
    calc, data = _images(ps, A, Imaging(defocus_series=(d, -d)))
    assert abs(calc._dz - d) < 1e-12
    plus, minus = data.image(0), data.image(1)
    contrast = oracle_B.std() / oracle_B.mean()
    e_orc, e_dev, e_minus = rel_l2(plus, oracle_B), rel_l2(plus, exits["B"]), rel_l2(minus, oracle_B)
    print(f"defocus +dz: vs oracle {e_orc:.3e}, vs msl_propagate {e_dev:.3e}; -dz: {e_minus:.3e}; contrast {contrast:.3f}")
    assert contrast >= 0.1
    assert e_orc <= 2e-4 and e_dev <= 2e-4
    assert e_minus > 2e-4 / contrast


def test_focal_spread(ps):
    """focal_points = 1 is bitwise the run without a focal spread; N = 5 is the NumPy sum over the nodes of the device's own exit
    spectra, to the bound of the kernel test"""
    from pyslice_amd import Aberrations, Imaging
    tr = _stack(6, 0.49, 2, seed=9)
    lens = dict(aberrations=Aberrations(Cs=1.0e7, C10=-400.0), aperture_mrad=25.0, defocus_series=(-100.0, 60.0))
    _, plain = _images(ps, tr, Imaging(**lens), frame_batch=2)
    _, one = _images(ps, tr, Imaging(focal_spread=30.0, focal_points=1, **lens), frame_batch=2)
    assert np.array_equal(one.intensity, plain.intensity)
    im5 = Imaging(focal_spread=30.0, focal_points=5, **lens)
    calc, five = _images(ps, tr, im5, frame_batch=2)
    ref = ps.MultisliceCalculator(progress=False, dtype="complex64", frame_batch=2)
    ref.setup(tr, aperture=0.0, voltage_eV=100e3)
    wfd = ref.run().wavefunction_data
    wf = (wfd.cpu().numpy() if hasattr(wfd, "cpu") else np.asarray(wfd))[0, :, :, :, 0]          # (T, nx, ny) complex64
    lam = ps.wavelength(100e3)
    kx, ky = np.fft.fftfreq(64, calc.dx)[:, None], np.fft.fftfreq(64, calc.dy)[None, :]
    spec = np.fft.ifftshift(wf.astype(np.complex128), axes=(-2, -1))
    _, w = im5.nodes()
    for f in range(2):
        want = sum(w[i] * (np.abs(np.fft.ifft2(spec * im5.transfer(kx, ky, lam, f=f, i=i), axes=(-2, -1))) ** 2).mean(axis=0) for i in range(5))
        err = rel_l2(five.image(f), want)
        print(f"focal spread, 5 nodes, defocus {f}: rel-L2 {err:.3e}; differs from the coherent image by {rel_l2(plain.image(f), want):.3e}")
        assert err <= image_tol((64, 64))


# ------------------------------------------------------------------ 4. end to end against the oracle
@pytest.fixture(scope="module")
def oracle_images(ps):
    from oracle import multislice_oracle as orc
    from pyslice_amd import Aberrations, Imaging
    from pyslice_amd.synthetic import synthetic_trajectory
    tr = synthetic_trajectory(96, 16, 3, ny=80, density=0.2, amplitude=0.1, seed=41, species=(79,))
    pp = [(2.0, 3.0), (5.5, 1.0)]
    ref = orc.run_frames(tr.box_matrix, tr.positions, tr.atom_types, 0.0, 100e3, pp, workers=orc.usable_cores())
    wf = ref["wavefunction_data"][..., 0]
    xs, ys = ref["xs"], ref["ys"]
    im = Imaging(aberrations=Aberrations(Cs=1.0e7), aperture_mrad=25.0, defocus_series=(-600.0, -430.0, -200.0))
    kx, ky = np.fft.fftfreq(len(xs), xs[1] - xs[0])[:, None], np.fft.fftfreq(len(ys), ys[1] - ys[0])[None, :]
    spec = np.fft.ifftshift(wf, axes=(-2, -1))
    want = np.stack([(np.abs(np.fft.ifft2(spec * im.transfer(kx, ky, orc.wavelength(100e3), f=f), axes=(-2, -1))) ** 2).mean(axis=1)
                     for f in range(3)], axis=1)                # (P, F, nx, ny)
    return tr, pp, im, want


def test_images_match_oracle(ps, oracle_images):
    """96 x 80 x 16 slices of gold at twice the density with 0.1 A displacements, 3 frames, plane wave, Cs = 1 mm, 25 mrad objective
    aperture (Nyquist is 185 mrad), defocus -600 / -430 / -200 A: every image to 2e-4 rel-L2 of the oracle's, whose contrast
    std / mean is 0.91, 0.74 and 0.63 (chosen on the CPU; asserted >= 0.1 so that the bound is not carried by the mean).  The same
    run at frame_batch 1 and 2 is bitwise equal; at probe_batch 1 it is equal to the run with both probes in one batch."""
    tr, pp, im, want = oracle_images
    assert want.shape == (2, 3, 96, 80)
    contrast = want.std(axis=(-2, -1)) / want.mean(axis=(-2, -1))
    print("oracle contrast std / mean per image:", np.round(contrast, 3).tolist())
    assert contrast.min() >= 0.1
    out = {}
    for fb, pb in ((1, 2), (2, 2), (2, 1)):
        calc, data = _images(ps, tr, im, pp=pp, frame_batch=fb, probe_batch=pb)
        assert calc._engine.frame_batch == fb and calc.probe_batch == pb
        assert data.intensity.shape == (2, 1, 3, 96, 80) and data.n_frames == 3
        out[fb, pb] = data.intensity[:, 0]
        errs = [rel_l2(out[fb, pb][p, f], want[p, f]) for p in range(2) for f in range(3)]
        print(f"frame_batch {fb} probe_batch {pb}: max rel-L2 per image {max(errs):.3e}")
        assert max(errs) <= 2e-4
    assert np.array_equal(out[1, 2], out[2, 2])                  # across frame batches: bitwise
    assert np.array_equal(out[2, 1], out[2, 2])                  # across probe batches
    assert np.array_equal(data.defocus, [-600.0, -430.0, -200.0]) and data.layer.tolist() == [15]

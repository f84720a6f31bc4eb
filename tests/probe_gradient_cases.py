"""The inputs, the float64 references and the bounds of the probe-parameter gradient tests (test_probe_gradient_host.py,
test_gpu_probe_gradient.py): the host test checks the fault sensitivity of the device bound on exactly the
inputs the device test runs.

Chain cases (msl_adjoint_probe_params on a given g0): 0.1 A pixels at 100 kV, three probes, a g0 white in both components (complex64
values), with the aberration set ABERR and with none.  The apertures give every disc but the first at least 100 pixels; on 12 x 1050
the aperture exceeds the grid along both axes, so the box is the whole grid with both Nyquist lines inside.

The bound is composed, not tuned: |got - want| <= (4 pi / N) ||b A||_2 tol ||ghat_p||_2 + 1e-12 sum |b| |ghat_p| per probe and basis
function b (adjoint.probe_parameter_bound), tol the two-pass contract of one 2-D transform: 3e-6 with both lengths 13-smooth, else
1e-5 (section 4.31)."""
import functools
from collections import namedtuple

import numpy as np

import gradient_cases as gc

DX = 0.1
PP = gc.PP
ChainCase = namedtuple("ChainCase", "name nx ny mrad")
CHAIN_CASES = [ChainCase("24x20", 24, 20, 30.0), ChainCase("45x63", 45, 63, 45.0), ChainCase("101x97", 101, 97, 30.0),
               ChainCase("96x80", 96, 80, 30.0), ChainCase("256x64", 256, 64, 30.0), ChainCase("64x256", 64, 256, 30.0),
               ChainCase("12x1050", 12, 1050, 200.0)]
RUN_GRIDS = [(96, 80, 4), (101, 97, 4)]
PM_TILE = 1024                              # adjoint.h: box pixels per tile of probe_moment_kernel
B_TERMS = [1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13]          # the terms with m > 0
FAULTS = ("ramp_sign", "swap_k", "no_1_over_N", "no_conj", "no_centre", "le_aperture", "nyquist_sign", "no_n_plus_1", "no_m", "swap_ab",
          "next_xy", "drop_pixel", "drop_last_tile")


def wavelength():
    return gc.orc.wavelength(gc.EV)


def aberr():
    from pyslice_amd import Aberrations
    return Aberrations(defocus=80.0, astigmatism=30.0, astigmatism_angle=0.4, coma=500.0, coma_angle=1.1, Cs=2.0e5)


def smooth13(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def fft_tol(nx, ny):
    return 3e-6 if smooth13(nx) and smooth13(ny) else 1e-5


def geometry(case):
    """the positional arguments of the adjoint.probe_* functions behind g0"""
    return case.nx, case.ny, DX, DX, wavelength(), case.mrad


@functools.lru_cache(maxsize=None)
def white_g0(case, P=3):
    rng = np.random.default_rng(case.nx * 7 + case.ny)
    g = (rng.standard_normal((P, case.nx, case.ny)) + 1j * rng.standard_normal((P, case.nx, case.ny))).astype(np.complex64)
    g.setflags(write=False)
    return g


def aperture_pixels(case):
    from pyslice_amd.adjoint import probe_aperture
    return int(probe_aperture(*geometry(case)).sum())


def pack(pos, per):
    """(P, 2), (P, 14, 2) -> (P, 30): the layout of msl_adjoint_probe_params"""
    return np.concatenate([pos, per.reshape(len(pos), 28)], axis=1)


@functools.lru_cache(maxsize=None)
def chain_reference(case, aberrated):
    """(want (3, 30), bound (3, 30)) float64"""
    from pyslice_amd.adjoint import probe_parameter_bound, probe_parameter_gradient
    g0 = white_g0(case)
    pos, _, per = probe_parameter_gradient(g0, *geometry(case), PP, aberr() if aberrated else None)
    return pack(pos, per), pack(*probe_parameter_bound(g0, *geometry(case), fft_tol(case.nx, case.ny)))


def ratio(got, want, bound):
    """the worst |got - want| / bound; a slot without a bound (b of an m = 0 term) must be zero"""
    dead = bound == 0
    assert not np.asarray(got)[dead].any() and not np.asarray(want)[dead].any()
    return float((np.abs(got - want)[~dead] / bound[~dead]).max())


def polar(cart30, ab, fault=None):
    """(P, 30) Cartesian rows -> (P, 2, 14): dL/dC and dL/dphi of every probe's share, the chain of adjoint.aberration_polar_gradient
    with the faults of the host test built in; |.| of the factors with absolute=True rows gives the bound"""
    from pyslice_amd.aberrations import TERMS
    lam = wavelength()
    pol = ab.as_polar()
    out = np.zeros((len(cart30), 2, 14))
    cart = cart30[:, 2:].reshape(-1, 14, 2)
    for j, (name, n, m) in enumerate(TERMS):
        c, phi = pol[j]
        w = 1.0 / ((1 if fault == "no_n_plus_1" else n + 1) * lam)
        out[:, 0, j] = (np.cos(m * phi) * cart[:, j, 0] + np.sin(m * phi) * cart[:, j, 1]) * w
        out[:, 1, j] = (1 if fault == "no_m" and m else m) * c * w * (-np.sin(m * phi) * cart[:, j, 0] + np.cos(m * phi) * cart[:, j, 1])
    return out


def polar_bound(bound30, ab):
    from pyslice_amd.aberrations import TERMS
    lam = wavelength()
    pol = ab.as_polar()
    out = np.zeros((len(bound30), 2, 14))
    b = bound30[:, 2:].reshape(-1, 14, 2)
    for j, (name, n, m) in enumerate(TERMS):
        c, phi = pol[j]
        w = 1.0 / ((n + 1) * lam)
        out[:, 0, j] = (abs(np.cos(m * phi)) * b[:, j, 0] + abs(np.sin(m * phi)) * b[:, j, 1]) * w
        out[:, 1, j] = m * abs(c) * w * (abs(np.sin(m * phi)) * b[:, j, 0] + abs(np.cos(m * phi)) * b[:, j, 1])
    return out


def box_axis(n, kfreq, radius):
    """mslice.hip: probe_box_axis -> (lo, w) in signed frequencies"""
    q = radius / kfreq
    reach = int(q) + 1 if q < n else n
    a, b = max(-reach, -(n // 2)), min(reach, (n - 1) // 2)
    return a, b - a + 1


def model(case, aberrated, fault=None, ghat=None):
    """(P, 30): the chain of probe_moment_kernel in NumPy float64 on the case's white g0 -- the definition when fault is None and ghat
    is None.  ghat: the transforms to use (a float32 transform's, for the precision model); fault: one of FAULTS, built in"""
    from pyslice_amd.adjoint import aberration_basis, aberration_cartesian
    nx, ny, dx, dy, lam, mrad = geometry(case)
    g0 = white_g0(case)
    if ghat is None:
        ghat = np.fft.fft2(g0.astype(np.complex128), axes=(-2, -1))
    xy = np.asarray(PP, dtype=np.float64)
    if fault == "next_xy":
        xy = np.roll(xy, -1, axis=0)
    fx = np.rint(np.fft.fftfreq(nx, 1.0 / nx))[:, None] + np.zeros((1, ny))
    fy = np.rint(np.fft.fftfreq(ny, 1.0 / ny))[None, :] + np.zeros((nx, 1))
    kx, ky = fx * (1.0 / (nx * dx)), fy * (1.0 / (ny * dy))
    radius = mrad * 1e-3 / lam
    k = np.sqrt(kx * kx + ky * ky)
    A = k <= radius if fault == "le_aperture" else k < radius
    basis = aberration_basis(kx, ky, lam)
    chi = np.tensordot(aberration_cartesian(aberr() if aberrated else None, lam), basis, axes=([0, 1], [0, 1]))
    if fault == "nyquist_sign":                             # the idealised shift: the Nyquist lines at +n/2
        fx = np.where((nx % 2 == 0) & (fx == -(nx // 2)), nx // 2, fx)
        fy = np.where((ny % 2 == 0) & (fy == -(ny // 2)), ny // 2, fy)
        kx, ky = fx * (1.0 / (nx * dx)), fy * (1.0 / (ny * dy))
    cen = 0.0 if fault == "no_centre" else 1.0
    t = fx * (cen * (nx // 2) / nx + xy[:, 0, None, None] / (nx * dx)) + fy * (cen * (ny // 2) / ny + xy[:, 1, None, None] / (ny * dy))
    if fault == "ramp_sign":
        t = -t
    Phi = A[None] * np.exp(2j * np.pi * (t - chi[None]))
    m = ((ghat if fault == "no_conj" else np.conj(ghat)) * Phi).imag
    if fault == "drop_pixel":
        i = np.argwhere(A)[len(np.argwhere(A)) // 2]
        m[:, i[0], i[1]] = 0.0
    if fault == "drop_last_tile":
        (xlo, wx), (ylo, wy) = box_axis(nx, 1.0 / (nx * dx), radius), box_axis(ny, 1.0 / (ny * dy), radius)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)   # the kernel's signed frequencies: fftfreq's
        q = (ix - xlo) * wy + (iy - ylo)
        inside = (ix >= xlo) & (ix < xlo + wx) & (iy >= ylo) & (iy < ylo + wy)
        assert inside[A].all()                              # the box holds the aperture
        last = ((wx * wy + PM_TILE - 1) // PM_TILE - 1) * PM_TILE
        m = m * ~(inside & (q >= last))[None]
    c = 4.0 * np.pi if fault == "no_1_over_N" else 4.0 * np.pi / (nx * ny)
    if fault == "swap_k":                                   # the axis lengths exchanged
        kx, ky = fx * (1.0 / (ny * dy)), fy * (1.0 / (nx * dx))
    pos = -c * np.stack([(kx[None] * m).sum(axis=(-2, -1)), (ky[None] * m).sum(axis=(-2, -1))], axis=1)
    per = c * np.einsum("jcxy,pxy->pjc", basis, m)
    if fault == "swap_ab":
        per = per[:, :, ::-1]
    return pack(pos, per)


def c64_ghat(case):
    """the transforms of the white g0 by a float32 FFT (torch, complex64), as complex128 values"""
    import torch
    return torch.fft.fft2(torch.from_numpy(np.array(white_g0(case)))).numpy().astype(np.complex128)


# ---- through the run: the physical inputs of gradient_cases ----
def run_geometry(grid):
    c = gc.case(*grid)
    xs, ys = c["xs"], c["ys"]
    return grid[0], grid[1], float(xs[1] - xs[0]), float(ys[1] - ys[0]), wavelength(), 30.0


@functools.lru_cache(maxsize=None)
def run_reference(grid, loss):
    """the full float64 definition at the setup of gradient_cases (no aberrations): dict(loss, probe, params (P, 30))"""
    from pyslice_amd.adjoint import probe_parameter_gradient
    ref = gc.reference(*grid, loss=loss)
    pos, _, per = probe_parameter_gradient(ref["probe"], *run_geometry(grid), PP)
    return dict(loss=ref["loss"], probe=ref["probe"], params=pack(pos, per), ref=ref)


def chain_bound_of(g0, grid):
    from pyslice_amd.adjoint import probe_parameter_bound
    return pack(*probe_parameter_bound(g0, *run_geometry(grid), fft_tol(grid[0], grid[1])))


def run_bound_b(grid, g0_ref):
    """(4 pi / N) ||b A||_2 sqrt N 3e-4 ||g0_p||_2 + the chain bound: the device's probe gradient is within 3e-4 rel-L2 of the
    definition's (what test_gpu_gradient.py holds), and ||ghat||_2 = sqrt N ||g0||_2"""
    from pyslice_amd.adjoint import probe_parameter_bound
    unit = pack(*probe_parameter_bound(g0_ref, *run_geometry(grid), 1.0))
    tiny = pack(*probe_parameter_bound(g0_ref, *run_geometry(grid), 0.0))
    return (unit - tiny) * 3e-4 + chain_bound_of(g0_ref, grid)


# ---- the directional derivative and the descent, chosen on the float64 model (grid RUN_GRIDS[0], the uploaded potential V) ----
def lens0():
    """the lens of the directional test: not the zero set, so that the polar chain and the override are on the path"""
    from pyslice_amd import Aberrations
    return Aberrations(defocus=60.0, astigmatism=25.0, astigmatism_angle=0.3, Cs=2.0e5)


# the direction, chosen on the float64 model so that <grad, d> is at least 5 tolerances there: every component moves, none against
# the slope
D_XY = np.array([[0.6, -0.1], [0.1, -0.8], [1.0, 0.5]])         # Angstrom per unit step
D_LENS = {"C10": 30.0, "C12": 20.0, "C30": 4.0e4}               # Angstrom per unit step: defocus, astigmatism, Cs
LENS_INDEX = {"C10": 0, "C12": 1, "C30": 4}


def lens_at(base, s, direction=D_LENS):
    import dataclasses
    from pyslice_amd import Aberrations
    f = {x.name: getattr(base, x.name) for x in dataclasses.fields(base)}
    for name, d in direction.items():
        f[name] += s * d
    return Aberrations(**f)


def model_run(grid, xy, lens, D, loss="amplitude"):
    """the float64 run at scan positions xy and an Aberrations: dict(loss (P,), Psi, probe, params (P, 30), bound (P, 30))"""
    from pyslice_amd import adjoint as adj
    c = gc.case(*grid)
    geom = run_geometry(grid)
    probes = np.fft.ifft2(adj.probe_spectrum(*geom, xy, lens), axes=(-2, -1))
    _, L, pg, det = adj.potential_gradient(probes, c["V"], D, c["sigma"], c["prop"], loss=loss, epsilon=gc.epsilon_of(c, loss), details=True)
    pos, _, per = adj.probe_parameter_gradient(pg, *geom, xy, lens)
    return dict(loss=L, Psi=det["Psi"], probe=pg, params=pack(pos, per), bound=chain_bound_of(pg, grid))


def loss_tolerance(grid, run, D, loss="amplitude"):
    """gradient_cases.loss_bound summed over the probes, for the data D"""
    c = dict(gc.case(*grid))
    c["D"] = D
    return float(gc.loss_bound(c, dict(Psi=run["Psi"], loss=run["loss"]), loss).sum())


def lens_inner(named, direction=D_LENS):
    return sum(named[k] * d for k, d in direction.items())


@functools.lru_cache(maxsize=None)
def directional64(grid=RUN_GRIDS[0]):
    """dict: h, the float64 central difference and <grad, d>, and the three terms of the tolerance (the loss bounds at the two ends
    over 2h, twice the truncation, the chain bound contracted with |d|); h is the largest of a few steps at which twice the
    truncation is below a tenth of the loss term"""
    from pyslice_amd.adjoint import aberration_polar_gradient
    D = gc.case(*grid)["D"]
    xy = np.asarray(PP, dtype=np.float64)
    base = model_run(grid, xy, lens0(), D)
    cart = base["params"][:, 2:].sum(axis=0).reshape(14, 2)
    dC, _ = aberration_polar_gradient(cart, lens0(), wavelength())
    inner = float((base["params"][:, :2] * D_XY).sum() + sum(dC[LENS_INDEX[k]] * d for k, d in D_LENS.items()))
    pb = polar_bound(base["bound"], lens0()).sum(axis=0)            # (2, 14): the probes' shares add
    chain = float((base["bound"][:, :2] * np.abs(D_XY)).sum() + sum(pb[0, LENS_INDEX[k]] * abs(d) for k, d in D_LENS.items()))
    for h in (0.02, 0.01, 0.005, 0.002, 0.001, 0.0005):
        ends = [model_run(grid, xy + s * h * D_XY, lens_at(lens0(), s * h), D) for s in (+1.0, -1.0)]
        fd = float(ends[0]["loss"].sum() - ends[1]["loss"].sum()) / (2.0 * h)
        loss_term = sum(loss_tolerance(grid, e, D) for e in ends) / (2.0 * h)
        if 2.0 * abs(fd - inner) <= 0.1 * loss_term:
            return dict(h=h, fd=fd, inner=inner, loss_term=loss_term, trunc=2.0 * abs(fd - inner), chain=chain)
    raise AssertionError("no step found")


SHIFT = 0.2 * np.array([[0.6, 0.8], [-0.8, 0.6], [1.0, 0.0]])   # every scan position displaced by 0.2 Angstrom
DEFOCUS_TRUE, DEFOCUS_OFF = 60.0, 20.0
RATE_XY, RATE_C10 = 5.0e-3, 12.0                               # chosen on the float64 model: about 0.4 of the Newton step


@functools.lru_cache(maxsize=None)
def descent_data(grid=RUN_GRIDS[0]):
    """the patterns of V at the true scan positions and the true defocus, (P, nx, ny) in the detector's layout"""
    from pyslice_amd import Aberrations
    from pyslice_amd import adjoint as adj
    c = gc.case(*grid)
    probes = np.fft.ifft2(adj.probe_spectrum(*run_geometry(grid), PP, Aberrations(defocus=DEFOCUS_TRUE)), axes=(-2, -1))
    D = np.fft.fftshift(np.abs(adj.forward_waves(probes, c["V"], c["sigma"], c["prop"])[2]) ** 2, axes=(-2, -1))
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def descent64(kind, grid=RUN_GRIDS[0]):
    """the float64 model of three plain descent steps, kind "positions" (from PP + SHIFT at the true defocus, rate RATE_XY) or
    "defocus" (from DEFOCUS_TRUE + DEFOCUS_OFF at the true positions, rate RATE_C10): (losses (4,), loss bounds (4,))"""
    from pyslice_amd import Aberrations
    from pyslice_amd.adjoint import aberration_polar_gradient
    D = descent_data(grid)
    xy, df = np.asarray(PP, dtype=np.float64) + (SHIFT if kind == "positions" else 0.0), DEFOCUS_TRUE + (DEFOCUS_OFF if kind == "defocus" else 0.0)
    losses, bounds = [], []
    for k in range(4):
        run = model_run(grid, xy, Aberrations(defocus=df), D)
        losses.append(float(run["loss"].sum()))
        bounds.append(loss_tolerance(grid, run, D))
        if kind == "positions":
            xy = xy - RATE_XY * run["params"][:, :2]
        else:
            cart = run["params"][:, 2:].sum(axis=0).reshape(14, 2)
            df = df - RATE_C10 * aberration_polar_gradient(cart, Aberrations(defocus=df), wavelength())[0][0]
    return np.array(losses), np.array(bounds)

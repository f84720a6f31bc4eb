"""The inputs and the float64 references of the gradient tests (test_gradient_host.py, test_gpu_gradient.py): the host test checks
the fault sensitivity of the device bounds on exactly the inputs the device tests run.

Cells as in test_gpu_absorptive.py / test_gpu_tds.py: 40 atoms per slice of Si and O, 0.1 A pixels, 1 A slices, 100 kV; 3 probes
(with probe_batch=2: one full batch and a ragged one).  The potential V is the oracle's, rounded to float32 (what potential=
uploads, so the device and the definition start from the same numbers); the data D are the patterns of 0.9 V."""
import functools

import numpy as np

from oracle import multislice_oracle as orc

EV = 100e3
EPS = 1e-4                                  # the rel-L2 the parity tests allow the waves
PP = [(3.05, 4.4), (1.7, 1.25), (4.1, 2.2)]
CASES = [(256, 64, 2), (64, 256, 4), (96, 80, 1), (96, 80, 4), (101, 97, 4)]
LOSSES = ("amplitude", "intensity", "poisson")
DIRECTION_H = 5.0                           # the step of the directional test along smooth_direction (unit maximum), in the units of V


@functools.lru_cache(maxsize=None)
def trajectory(nx, ny, nz):
    from pyslice_amd import Trajectory
    from pyslice_amd.synthetic import box_for_grid
    box = box_for_grid(nx, nz, 0.1, 1.0, ny)
    rng = np.random.default_rng(nx + ny + nz)
    n = 40 * nz
    pos = rng.random((n, 3)) * np.array([box[0, 0], box[1, 1], box[2, 2]])
    Z = np.array([14, 8], dtype=np.int32)[rng.integers(0, 2, n)]
    return Trajectory(atom_types=Z, positions=pos[None], velocities=np.zeros((1, n, 3)), box_matrix=box, timestep=1.0)


@functools.lru_cache(maxsize=None)
def case(nx, ny, nz):
    """dict: the axes, sigma, the propagator, the probes, V (nz, nx, ny) float64 holding float32 values, and the data D (P, nx, ny)
    in the detector's layout; read-only"""
    import pyslice_amd
    from pyslice_amd.adjoint import forward_waves
    from pyslice_amd.tilt import tilted_propagator
    tr = trajectory(nx, ny, nz)
    xs, ys, zs = pyslice_amd.gridFromTrajectory(tr, 0.1, 1.0)[:3]
    assert (len(xs), len(ys), len(zs)) == (nx, ny, nz)
    V = np.moveaxis(orc.potential(xs, ys, zs, tr.positions[0], tr.atom_types), 2, 0).astype(np.float32).astype(np.float64)
    sigma = orc.interaction_sigma(EV)
    prop = tilted_propagator(nx, ny, xs[1] - xs[0], ys[1] - ys[0], orc.wavelength(EV), zs[1] - zs[0] if nz > 1 else 0.5, None)
    probes = orc.batched_probes(orc.probe_array(xs, ys, 30.0, EV), xs, ys, PP)
    V09 = (0.9 * V).astype(np.float32).astype(np.float64)
    D = np.fft.fftshift(np.abs(forward_waves(probes, V09, sigma, prop)[2]) ** 2, axes=(-2, -1))
    out = dict(xs=xs, ys=ys, zs=zs, sigma=sigma, prop=prop, probes=probes, V=V, V09=V09, D=D)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def poisson_epsilon(c):
    """the floor of the Poisson tests: 1e-6 of a pattern's sum (the loss bound's series in eta / (I + eps) needs eps >= 4 EPS^2 sum I)"""
    return 1e-6 * float(c["D"][0].sum())


def epsilon_of(c, loss):
    return poisson_epsilon(c) if loss == "poisson" else 1e-20


def disc_weight(nx, ny):
    """1 inside a disc of 0.4 of the shorter half axis around the centre of the detector, 0 outside; (nx, ny) float32"""
    x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
    return ((x * x + y * y) <= (0.4 * min(nx, ny) / 2) ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(nx, ny, nz, loss="amplitude", weighted=False, start="V"):
    """the float64 definition at V (or at 0.9 V: start="V09"): grad, loss, probe gradient and the intermediate waves"""
    from pyslice_amd.adjoint import potential_gradient
    c = case(nx, ny, nz)
    w = disc_weight(nx, ny) if weighted else None
    grad, L, pg, det = potential_gradient(c["probes"], c[start], c["D"], c["sigma"], c["prop"], loss=loss, weight=w,
                                          epsilon=epsilon_of(c, loss), details=True)
    return dict(grad=grad, loss=L, probe=pg, **det)


def gradient_bound(c, ref):
    """(nz,): 3 EPS 2 sigma sum_p ||g_p,s||_2 ||phi_p,s||_2 -- Cauchy-Schwarz on the pixelwise product Im(g conj phi): each factor
    carries EPS, and the adjoint wave has been through both loops"""
    return np.array([3.0 * EPS * 2.0 * c["sigma"] * sum(np.linalg.norm(g[p]) * np.linalg.norm(phi[p]) for p in range(len(g)))
                     for g, phi in ref["pairs"]])


def loss_bound(c, ref, loss, weight=None):
    """(P,): the change of the loss when the exit amplitudes a = |Psi| move by delta with ||delta||_2 <= EPS ||a||_2 (S = sum I):
    amplitude   dL = sum 2 (a - sqrt D) delta + delta^2                    <= 2 EPS sqrt(L S) + EPS^2 S
    intensity   eta = I' - I = 2 a delta + delta^2, ||eta||_2 <= E = 2 EPS max(a) sqrt(S) + EPS^2 S;
                dL = sum (I - D) eta + eta^2 / 2                           <= sqrt(2 L) E + E^2 / 2
    poisson     dL = sum eta - D log(1 + x), x = eta / (I + eps), |log(1 + x) - x| <= x^2 for |x| <= 1/2 (which eps >= 4 EPS^2 S
                gives): |sum eta| <= (2 EPS + EPS^2) S; sum D |x| <= 2 ||D a / (I + eps)||_2 EPS sqrt(S) + max(D / (I + eps)) EPS^2 S;
                sum D x^2 <= 5 max(D / (I + eps)) EPS^2 S
                                                                           <= 2 EPS sqrt(S) (sqrt(S) + ||D a / (I + eps)||_2)
                                                                              + EPS^2 S (1 + 6 max(D / (I + eps)))
    With a weight 0 <= w <= 1 the sums run over fewer terms: the bounds hold as they are."""
    I = np.abs(ref["Psi"]) ** 2
    S = I.sum(axis=(1, 2))
    L = np.abs(ref["loss"])
    if loss == "amplitude":
        return 2.0 * EPS * np.sqrt(L * S) + EPS ** 2 * S
    if loss == "intensity":
        E = 2.0 * EPS * np.sqrt(I.max(axis=(1, 2))) * np.sqrt(S) + EPS ** 2 * S
        Lsq = 0.5 * ((I - np.fft.ifftshift(c["D"], axes=(-2, -1))) ** 2).sum(axis=(1, 2))       # (the unweighted loss: an upper bound)
        return np.sqrt(2.0 * Lsq) * E + 0.5 * E ** 2
    eps = epsilon_of(c, loss)
    D = np.fft.ifftshift(c["D"], axes=(-2, -1))
    r = D / (I + eps)
    return (2.0 * EPS * np.sqrt(S) * (np.sqrt(S) + np.sqrt(((r * np.sqrt(I)) ** 2).sum(axis=(1, 2))))
            + EPS ** 2 * S * (1.0 + 6.0 * r.max(axis=(1, 2))))


def smooth_direction(nx, ny, nz, seed=5):
    """a smooth random direction (nz, nx, ny) of unit maximum: a few low Fourier modes per slice"""
    rng = np.random.default_rng(seed)
    spec = np.zeros((nz, nx, ny), dtype=np.complex128)
    spec[:, :4, :4] = rng.standard_normal((nz, 4, 4)) + 1j * rng.standard_normal((nz, 4, 4))
    d = np.fft.ifft2(spec, axes=(-2, -1)).real
    return d / np.abs(d).max()

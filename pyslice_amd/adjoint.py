"""The slice loop backwards, in float64 NumPy: the definition of MultisliceCalculator(gradient=...) / run_gradient() and of the
msl_adjoint_* entry points.

Forward, for a probe psi_0 and the slice potentials V_s (t_s = exp(i sigma V_s), P the propagator on numpy's fftfreq grid):
    phi_s = t_s psi_s,    psi_{s+1} = ifft2(P fft2 phi_s)  (s < nz - 1),    Psi = fft2(phi_{nz-1}),    I = |Psi|^2
-- I in the transform's own order; the data D and the weight w are in the detector's layout (fftshifted), as
DiffractionData.intensity of an unbinned, unwindowed run.

Loss per probe, and its residual G = dL/dPsi* (dL = 2 Re sum conj(G) dPsi):
    "amplitude"   L = sum w (sqrt I - sqrt D)^2          G = w (1 - sqrt D / max(|Psi|, sqrt eps)) Psi
    "intensity"   L = 1/2 sum w (I - D)^2                G = w (I - D) Psi
    "poisson"     L = sum w (I - D log(I + eps))         G = w (1 - D / (I + eps)) Psi

Backward: g = N ifft2(G), N = nx ny (the adjoint of the unnormalised fft2); for s = nz - 1 .. 0:
    dL/dV_s += 2 sigma sum_p Im(g_p conj(phi_p,s)),    g <- conj(t_s) g,    and for s > 0    g <- ifft2(conj(P) fft2 g).
After s = 0, g is dL/dpsi_0* per probe: the probe gradient."""
from __future__ import annotations

import numpy as np

LOSSES = {"amplitude": 1, "intensity": 2, "poisson": 3}         # include/mslice.h: MSL_ADJ_*

_AX = (-2, -1)


def _check_loss(loss):
    if loss not in LOSSES:
        raise ValueError(f"gradient: loss must be one of {sorted(LOSSES)}, got {loss!r}")


def forward_waves(probes, V, sigma, prop):
    """probes (P, nx, ny) complex, V (nz, nx, ny) real, prop (nx, ny) complex -> (psi, phi, Psi): the waves arriving at every slice
    and behind its transmission, (nz, P, nx, ny) complex128 each, and the exit spectra fft2(phi[nz - 1]), (P, nx, ny), unshifted"""
    psi = np.array(probes, dtype=np.complex128)
    if psi.ndim == 2:
        psi = psi[None]
    V = np.asarray(V, dtype=np.float64)
    if V.ndim != 3 or V.shape[1:] != psi.shape[1:]:
        raise ValueError(f"forward_waves: V {V.shape} does not match the waves {psi.shape}: expected (nz, nx, ny)")
    nz = V.shape[0]
    psis, phis = np.empty((nz,) + psi.shape, dtype=np.complex128), np.empty((nz,) + psi.shape, dtype=np.complex128)
    for s in range(nz):
        psis[s] = psi
        phis[s] = np.exp(1j * sigma * V[s])[None] * psi
        if s < nz - 1:
            psi = np.fft.ifft2(prop[None] * np.fft.fft2(phis[s], axes=_AX), axes=_AX)
    return psis, phis, np.fft.fft2(phis[nz - 1], axes=_AX)


def loss_and_residual(Psi, data, loss="amplitude", weight=None, epsilon=1e-20):
    """Psi (P, nx, ny) unshifted exit spectra; data (P, nx, ny) and weight (nx, ny) or None in the detector's (fftshifted) layout
    -> (L (P,) float64, G (P, nx, ny) complex128, unshifted)"""
    _check_loss(loss)
    Psi = np.asarray(Psi, dtype=np.complex128)
    D = np.fft.ifftshift(np.asarray(data, dtype=np.float64), axes=_AX)
    if D.shape != Psi.shape:
        raise ValueError(f"gradient: data {D.shape} does not match the patterns {Psi.shape}")
    w = 1.0 if weight is None else np.fft.ifftshift(np.asarray(weight, dtype=np.float64))[None]
    I = np.abs(Psi) ** 2
    if loss == "amplitude":
        a, sd = np.sqrt(I), np.sqrt(D)
        L = (w * (a - sd) ** 2).sum(axis=_AX)
        G = w * (1.0 - sd / np.maximum(a, np.sqrt(epsilon))) * Psi
    elif loss == "intensity":
        L = 0.5 * (w * (I - D) ** 2).sum(axis=_AX)
        G = w * (I - D) * Psi
    else:
        L = (w * (I - D * np.log(I + epsilon))).sum(axis=_AX)
        G = w * (1.0 - D / (I + epsilon)) * Psi
    return L, G


def backward(G, psis, V, sigma, prop, phi_of=None):
    """the backward loop for the residual G (P, nx, ny) and the forward waves psis (nz, P, nx, ny) -> (grad (nz, nx, ny) float64, the
    probe gradient (P, nx, ny) complex128, and per slice the pairs (g, phi) the product was formed from)"""
    V = np.asarray(V, dtype=np.float64)
    nz, npix = V.shape[0], V.shape[1] * V.shape[2]
    g = npix * np.fft.ifft2(G, axes=_AX)
    grad = np.zeros(V.shape, dtype=np.float64)
    pairs = [None] * nz
    for s in range(nz - 1, -1, -1):
        t = np.exp(1j * sigma * V[s])[None]
        phi = t * psis[s]
        pairs[s] = (g.copy(), phi)
        grad[s] = 2.0 * sigma * (g * np.conj(phi)).imag.sum(axis=0)
        g = np.conj(t) * g
        if s > 0:
            g = np.fft.ifft2(np.conj(prop)[None] * np.fft.fft2(g, axes=_AX), axes=_AX)
    return grad, g, pairs


def potential_gradient(probes, V, data, sigma, prop, loss="amplitude", weight=None, epsilon=1e-20, details=False):
    """probes (P, nx, ny), V (nz, nx, ny), data (P, nx, ny) in the detector's layout -> (grad (nz, nx, ny) float64 = dL/dV summed over
    the probes, loss (P,), probe_grad (P, nx, ny) complex128 = dL/dpsi_0*); with details=True also a dict of the intermediate waves
    (psi, Psi, G, and per slice the pairs (g, phi)): what the bounds of the device tests are made from"""
    psis, phis, Psi = forward_waves(probes, V, sigma, prop)
    L, G = loss_and_residual(Psi, data, loss, weight, epsilon)
    grad, pg, pairs = backward(G, psis, V, sigma, prop)
    if details:
        return grad, L, pg, dict(psi=psis, Psi=Psi, G=G, pairs=pairs)
    return grad, L, pg


def total_loss(probes, V, data, sigma, prop, loss="amplitude", weight=None, epsilon=1e-20):
    """the loss alone, summed over the probes"""
    return float(loss_and_residual(forward_waves(probes, V, sigma, prop)[2], data, loss, weight, epsilon)[0].sum())


def directional_check(probes, V, data, sigma, prop, direction, h, loss="amplitude", weight=None, epsilon=1e-20):
    """(fd, inner): the central difference (L(V + h d) - L(V - h d)) / 2h of the total loss along `direction` (nz, nx, ny), and
    <grad, d> from potential_gradient"""
    d = np.asarray(direction, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    kw = dict(loss=loss, weight=weight, epsilon=epsilon)
    fd = (total_loss(probes, V + h * d, data, sigma, prop, **kw) - total_loss(probes, V - h * d, data, sigma, prop, **kw)) / (2.0 * h)
    return fd, float((potential_gradient(probes, V, data, sigma, prop, **kw)[0] * d).sum())


# ---- gradients with respect to atom positions: the potential build backwards ----
# Forward (oracle.potential): V_s = Re ifft2( sum_Z f_Z(q^2) sum_{a in Z, s} e^{-2 pi i (kx x_a + ky y_a)} ) / (dx^2 dy^2) on numpy's fftfreq
# grid; atom a belongs to slice s by slice_edges.  With Gamma_s = dL/dV_s, B_s = fft2(Gamma_s), N = nx ny, c = 2 pi / (N dx^2 dy^2):
#     dL/dx_a = c sum_{kx, ky} kx f_Z(k) Im( conj(B_s(k)) e^{-2 pi i kx x_a} e^{-2 pi i ky y_a} ),    dL/dy_a: the same with ky
# over the FULL grid (on an even length the Nyquist line has one sign and no mirror image).  The derivative along the slice axis is zero
# (an atom is binned, not spread), and an atom in no slice gets zeros.

def _position_setup(xs, ys, zs, positions, Z, dLdV, slice_axis):
    from .potentials import slice_edges
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    pos = np.asarray(positions, dtype=np.float64)
    Z = np.asarray(Z)
    if pos.ndim != 2 or pos.shape[1] != 3 or Z.shape != (pos.shape[0],):
        raise ValueError(f"position_gradient: positions {pos.shape} must be (n_atoms, 3) with one atomic number per atom")
    if slice_axis not in (0, 1, 2):
        raise ValueError(f"position_gradient: slice_axis must be 0, 1 or 2, got {slice_axis}")
    nx, ny = len(xs), len(ys)
    lo, hi = slice_edges([xs, ys, zs][slice_axis])
    G = np.asarray(dLdV, dtype=np.float64)
    if G.shape != (len(lo), nx, ny):
        raise ValueError(f"position_gradient: dLdV {G.shape} does not match ({len(lo)}, {nx}, {ny}): (slices, nx, ny)")
    axes = [0, 1, 2]
    axes.remove(slice_axis)
    zc = pos[:, slice_axis]
    inside = (zc[:, None] >= lo[None, :]) & (zc[:, None] < hi[None, :])
    s_of = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    kx, ky = np.fft.fftfreq(nx, d=dx), np.fft.fftfreq(ny, d=dy)
    return pos, Z, G, axes, s_of, kx, ky, 2.0 * np.pi / (nx * ny * dx * dx * dy * dy)


def _form_factors(Z, kx, ky, table):
    from .potentials import loadKirkland
    table = loadKirkland() if table is None else np.asarray(table, dtype=np.float64).reshape(103, 3, 4)
    q2 = kx[:, None] ** 2 + ky[None, :] ** 2
    out = {}
    for z in np.unique(Z):
        t = table[int(z) - 1]
        out[int(z)] = sum(a / (q2 + b) for a, b, c, d in t) + sum(c * np.exp(-d * q2) for a, b, c, d in t)
    return out


def position_gradient(xs, ys, zs, positions, Z, dLdV, slice_axis=2, table=None):
    """dLdV (slices, nx, ny) real = dL/dV_s -> (n_atoms, 3) float64 = dL/dr_a in the caller's axes: the two in-plane columns by the
    formula above, the slice-axis column zero, zero rows for atoms in no slice.  xs, ys, zs, slice_axis as oracle.potential takes them
    (the slices are [xs, ys, zs][slice_axis], the in-plane coordinates the two other columns in order); table: a (103, 3, 4)
    form-factor table in place of Kirkland's."""
    pos, Z, G, axes, s_of, kx, ky, c = _position_setup(xs, ys, zs, positions, Z, dLdV, slice_axis)
    ff = _form_factors(Z, kx, ky, table)
    out = np.zeros((len(pos), 3), dtype=np.float64)
    for s in np.unique(s_of[s_of >= 0]):
        Bc = np.conj(np.fft.fft2(G[s]))
        for z, f in ff.items():
            idx = np.nonzero((s_of == s) & (Z == z))[0]
            if not len(idx):
                continue
            W = f * Bc
            ex = np.exp(-2j * np.pi * np.outer(pos[idx, axes[0]], kx))          # (a, nx)
            ey = np.exp(-2j * np.pi * np.outer(pos[idx, axes[1]], ky))          # (a, ny)
            out[idx, axes[0]] = c * ((ex * kx[None]) * (ey @ W.T)).sum(axis=1).imag
            out[idx, axes[1]] = c * (ex * ((ey * ky[None]) @ W.T)).sum(axis=1).imag
    return out


def position_gradient_bound(xs, ys, zs, positions, Z, dLdV, slice_axis=2, table=None):
    """(n_atoms, 2): c sum_k |kx| |f_Z| |B_s| and the same with |ky| -- the sums of the absolute terms of position_gradient, which the
    tolerances of the device tests are stated against; zero rows for atoms in no slice"""
    pos, Z, G, axes, s_of, kx, ky, c = _position_setup(xs, ys, zs, positions, Z, dLdV, slice_axis)
    ff = _form_factors(Z, kx, ky, table)
    out = np.zeros((len(pos), 2), dtype=np.float64)
    for s in np.unique(s_of[s_of >= 0]):
        Ba = np.abs(np.fft.fft2(G[s]))
        for z, f in ff.items():
            m = (s_of == s) & (Z == z)
            W = np.abs(f) * Ba
            out[m, 0] = c * (np.abs(kx)[:, None] * W).sum()
            out[m, 1] = c * (np.abs(ky)[None, :] * W).sum()
    return out


def position_loss(xs, ys, zs, positions, Z, probes, data, sigma, prop, loss="amplitude", weight=None, epsilon=1e-20, slice_axis=2):
    """the total loss of the patterns of the structure `positions`: oracle.potential's formula (float64), then total_loss"""
    return total_loss(probes, _potential_of(xs, ys, zs, positions, Z, slice_axis), data, sigma, prop, loss, weight, epsilon)


def _potential_of(xs, ys, zs, positions, Z, slice_axis=2, table=None):
    """V (slices, nx, ny) float64 of the forward formula above"""
    n_sl = len([xs, ys, zs][slice_axis])
    pos, Z, _, axes, s_of, kx, ky, c = _position_setup(xs, ys, zs, positions, Z, np.zeros((n_sl, len(xs), len(ys))), slice_axis)
    ff = _form_factors(Z, kx, ky, table)
    R = np.zeros((n_sl, len(xs), len(ys)), dtype=np.complex128)
    for s in np.unique(s_of[s_of >= 0]):
        for z, f in ff.items():
            idx = np.nonzero((s_of == s) & (Z == z))[0]
            if len(idx):
                R[s] += f * (np.exp(-2j * np.pi * np.outer(kx, pos[idx, axes[0]])) @ np.exp(-2j * np.pi * np.outer(pos[idx, axes[1]], ky)))
    return np.fft.ifft2(R, axes=_AX).real * (c * len(xs) * len(ys) / (2.0 * np.pi))


def position_directional_check(xs, ys, zs, positions, Z, probes, data, sigma, prop, direction, h, loss="amplitude", weight=None,
                               epsilon=1e-20, slice_axis=2):
    """(fd, inner): the central difference (L(r + h d) - L(r - h d)) / 2h of the total loss under positions +- h direction, and
    <grad, d> with grad = position_gradient of potential_gradient at `positions`"""
    pos = np.asarray(positions, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64)
    kw = dict(loss=loss, weight=weight, epsilon=epsilon)
    L = lambda r: position_loss(xs, ys, zs, r, Z, probes, data, sigma, prop, slice_axis=slice_axis, **kw)
    fd = (L(pos + h * d) - L(pos - h * d)) / (2.0 * h)
    dLdV = potential_gradient(probes, _potential_of(xs, ys, zs, pos, Z, slice_axis), data, sigma, prop, **kw)[0]
    return fd, float((position_gradient(xs, ys, zs, pos, Z, dLdV, slice_axis) * d).sum())


class Gradient:
    """MultisliceCalculator(gradient=Gradient(...)): run_gradient(data) returns dL/dV of the loss between the run's exit patterns
    and `data`.  loss: "amplitude", "intensity" or "poisson"; weight: (nx, ny) >= 0 in the detector's layout, or None; epsilon: the
    floor of |Psi|^2 in the amplitude and Poisson residuals; probe=True also returns dL/dpsi_0* per probe; positions=True also
    returns dL/dr_a per atom (GradientData.positions: the potential build backwards, section 4.32)."""

    def __init__(self, loss="amplitude", weight=None, epsilon=1e-20, probe=False, positions=False):
        _check_loss(loss)
        with np.errstate(over="ignore", under="ignore"):
            e32 = np.float32(epsilon)                           # (what the kernels hold: it must not round to zero or overflow there)
        if not (np.isfinite(e32) and e32 > 0):
            raise ValueError(f"gradient: epsilon must be a finite float32 number > 0, got {epsilon!r}")
        if weight is not None:
            weight = np.array(weight, dtype=np.float32)
            if weight.ndim != 2 or not np.isfinite(weight).all() or (weight < 0).any():
                raise ValueError("gradient: weight must be a finite (nx, ny) array >= 0")
            weight.setflags(write=False)
        self.loss, self.weight, self.epsilon, self.probe = loss, weight, float(epsilon), bool(probe)
        self.positions = bool(positions)

    @property
    def kind(self):
        return LOSSES[self.loss]

    def __repr__(self):
        return (f"Gradient(loss={self.loss!r}, weight={'None' if self.weight is None else self.weight.shape}, epsilon={self.epsilon:g}, "
                f"probe={self.probe}" + (", positions=True" if self.positions else "") + ")")

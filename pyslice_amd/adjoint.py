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


# ---- gradients with respect to scan positions and probe aberrations: the probe recipe backwards ----
# The device builds (probe_kspace_kernel / probe_kspace_aberr_kernel) psi0_p = ifft2(Phi_p),
#     Phi_p(k) = A(k) exp(2 pi i (t_p(k) - chi(k) / 2 pi)),
#     A          the strict aperture rule sqrt(kx^2 + ky^2) < mrad 1e-3 / lambda, kx = fx / Lx, ky = fy / Ly on signed indices fx, fy
#                (fftfreq's: on an even length the Nyquist line is f = -n/2),
#     t_p        = fx (floor(nx/2)/nx + x_p/Lx) + fy (floor(ny/2)/ny + y_p/Ly),
#     chi / 2 pi = sum_j a_j A_j(k) + b_j B_j(k),   A_j = (alpha^2)^((n+1-m)/2) Re z^m,  B_j = ... Im z^m,  z = lambda (kx + i ky),
#     (a_j, b_j) = C_nm (cos, sin)(m phi_nm) / ((n + 1) lambda)                                        (aberration.h, fourteen terms).
# With g0 = dL/dpsi0* (dL = 2 Re sum_r conj(g0) dpsi0), ghat = fft2(g0) and N = nx ny: dpsi0 = ifft2(dPhi) gives
# dL = (2/N) Re sum_k conj(ghat) dPhi.  dPhi/dx_p = 2 pi i kx Phi, dPhi/da_j = -2 pi i A_j Phi, and Re(i w) = -Im(w), so with the real
# field m_p(k) = Im(conj(ghat(k)) Phi_p(k))
#     dL/dx_p = -(4 pi / N) sum_k kx m_p(k),     dL/da_j = +(4 pi / N) sum_p sum_k A_j(k) m_p(k)     (ky and B_j likewise);
#     dL/dC_nm   = (cos(m phi) dL/da + sin(m phi) dL/db) / ((n + 1) lambda),
#     dL/dphi_nm = m C_nm / ((n + 1) lambda) (-sin(m phi) dL/da + cos(m phi) dL/db).
# The ramp is differentiated as it is built: on an even length the Nyquist line carries kx = -n/(2 Lx) and no mirror image.

def _probe_grid(nx, ny, dx, dy):
    fx = np.rint(np.fft.fftfreq(nx, 1.0 / nx))[:, None]
    fy = np.rint(np.fft.fftfreq(ny, 1.0 / ny))[None, :]
    return fx, fy, fx * (1.0 / (nx * dx)), fy * (1.0 / (ny * dy))


def aberration_cartesian(aberrations, wavelength):
    """(14, 2) float64: (a_j, b_j) of an Aberrations (None: zeros), as probe_aberrations (aberration.h) makes them"""
    from .aberrations import TERMS
    out = np.zeros((14, 2), dtype=np.float64)
    if aberrations is not None:
        for j, ((name, n, m), (c, phi)) in enumerate(zip(TERMS, aberrations.as_polar())):
            w = c / ((n + 1) * wavelength)
            out[j] = (w * np.cos(m * phi), w * np.sin(m * phi)) if m else (w, 0.0)
    return out


def aberration_basis(kx, ky, wavelength):
    """(14, 2, nx, ny) float64: A_j(k) and B_j(k), the factors of a_j and b_j in chi / 2 pi (B of an m = 0 term is zero)"""
    from .aberrations import TERMS
    z = wavelength * (kx + 1j * ky)
    r2 = np.abs(z) ** 2
    out = np.zeros((14, 2) + z.shape, dtype=np.float64)
    for j, (name, n, m) in enumerate(TERMS):
        zm = r2 ** ((n + 1 - m) // 2) * z ** m
        out[j, 0], out[j, 1] = zm.real, zm.imag
    return out


def probe_aperture(nx, ny, dx, dy, wavelength, mrad):
    """(nx, ny) bool: the strict aperture rule of the probe kernels"""
    _, _, kx, ky = _probe_grid(nx, ny, dx, dy)
    return np.sqrt(kx * kx + ky * ky) < (mrad * 1e-3) / wavelength


def probe_spectrum(nx, ny, dx, dy, wavelength, mrad, xy, aberrations=None, cartesian=None):
    """Phi (P, nx, ny) complex128 of the probes at xy (P, 2): ifft2 of it is what msl_set_probes builds.  aberrations: an Aberrations
    or None; cartesian: (14, 2) coefficients (a_j, b_j) in its place"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    fx, fy, kx, ky = _probe_grid(nx, ny, dx, dy)
    ab = aberration_cartesian(aberrations, wavelength) if cartesian is None else np.asarray(cartesian, dtype=np.float64)
    chi = np.tensordot(ab, aberration_basis(kx, ky, wavelength), axes=([0, 1], [0, 1]))
    t = (fx * ((nx // 2) / nx + xy[:, 0, None, None] / (nx * dx)) + fy * ((ny // 2) / ny + xy[:, 1, None, None] / (ny * dy))) - chi[None]
    return probe_aperture(nx, ny, dx, dy, wavelength, mrad)[None] * np.exp(2j * np.pi * (t - np.rint(t)))


def _probe_moment_fields(g0, nx, ny, dx, dy, wavelength, mrad, xy, aberrations, cartesian):
    g0 = np.asarray(g0, dtype=np.complex128)
    if g0.ndim == 2:
        g0 = g0[None]
    Phi = probe_spectrum(nx, ny, dx, dy, wavelength, mrad, xy, aberrations, cartesian)
    if g0.shape != Phi.shape:
        raise ValueError(f"probe_parameter_gradient: g0 {g0.shape} does not match the probes {Phi.shape}")
    _, _, kx, ky = _probe_grid(nx, ny, dx, dy)
    ghat = np.fft.fft2(g0, axes=_AX)
    return ghat, Phi, kx + 0 * ky, ky + 0 * kx, aberration_basis(kx, ky, wavelength)


def probe_parameter_gradient(g0, nx, ny, dx, dy, wavelength, mrad, xy, aberrations=None, cartesian=None):
    """g0 (P, nx, ny) complex = dL/dpsi0* -> (pos (P, 2) = dL/d(x_p, y_p), cart (14, 2) = dL/d(a_j, b_j) summed over the probes, which
    share the lens, per_probe (P, 14, 2)), float64, by the formulas above"""
    ghat, Phi, kx, ky, basis = _probe_moment_fields(g0, nx, ny, dx, dy, wavelength, mrad, xy, aberrations, cartesian)
    m = (np.conj(ghat) * Phi).imag
    c = 4.0 * np.pi / (nx * ny)
    pos = -c * np.stack([(kx[None] * m).sum(axis=_AX), (ky[None] * m).sum(axis=_AX)], axis=1)
    per = c * np.einsum("jcxy,pxy->pjc", basis, m)
    return pos, per.sum(axis=0), per


def probe_parameter_bound(g0, nx, ny, dx, dy, wavelength, mrad, tol, ghat=None):
    """(pos (P, 2), cart (P, 14, 2)): (4 pi / N) ||b A||_2 tol ||ghat_p||_2 + 1e-12 sum_k |b| |ghat_p| over the aperture A, per probe and
    basis function b (kx, ky, A_j, B_j) -- Cauchy-Schwarz on the moment of a transform that carries the relative L2 error tol; the
    second term is the float64 sum's own.  ghat: the transforms themselves in place of g0"""
    if ghat is None:
        ghat = np.fft.fft2(np.asarray(g0, dtype=np.complex128), axes=_AX)
    ghat = np.abs(ghat if ghat.ndim == 3 else ghat[None])
    _, _, kx, ky = _probe_grid(nx, ny, dx, dy)
    A = probe_aperture(nx, ny, dx, dy, wavelength, mrad)
    b = np.concatenate([np.stack([kx + 0 * ky, ky + 0 * kx]), aberration_basis(kx, ky, wavelength).reshape(28, nx, ny)]) * A[None]
    norm = np.sqrt((ghat ** 2).sum(axis=_AX))
    out = (4.0 * np.pi / (nx * ny)) * np.sqrt((b ** 2).sum(axis=_AX))[None, :] * tol * norm[:, None] \
        + 1e-12 * np.einsum("bxy,pxy->pb", np.abs(b), ghat)
    return out[:, :2], out[:, 2:].reshape(-1, 14, 2)


def aberration_polar_gradient(cart, aberrations, wavelength):
    """cart (14, 2) = dL/d(a_j, b_j) -> (dC (14,), dphi (14,)): dL/dC_nm per Angstrom and dL/dphi_nm per radian at `aberrations`
    (None: all zero, where dphi is zero and dC is dL/da)"""
    from .aberrations import TERMS
    cart = np.asarray(cart, dtype=np.float64)
    polar = np.zeros((14, 2)) if aberrations is None else aberrations.as_polar()
    dC, dphi = np.zeros(14), np.zeros(14)
    for j, (name, n, m) in enumerate(TERMS):
        c, phi = polar[j]
        w = 1.0 / ((n + 1) * wavelength)
        dC[j] = (np.cos(m * phi) * cart[j, 0] + np.sin(m * phi) * cart[j, 1]) * w
        dphi[j] = m * c * w * (-np.sin(m * phi) * cart[j, 0] + np.cos(m * phi) * cart[j, 1])
    return dC, dphi


def probe_loss(nx, ny, dx, dy, wavelength, mrad, xy, V, data, sigma, prop, aberrations=None, cartesian=None, loss="amplitude",
               weight=None, epsilon=1e-20):
    """the total loss of the patterns of the probes of this recipe"""
    probes = np.fft.ifft2(probe_spectrum(nx, ny, dx, dy, wavelength, mrad, xy, aberrations, cartesian), axes=_AX)
    return total_loss(probes, V, data, sigma, prop, loss, weight, epsilon)


def probe_directional_check(nx, ny, dx, dy, wavelength, mrad, xy, V, data, sigma, prop, d_xy, d_cart, h, aberrations=None, cartesian=None,
                            loss="amplitude", weight=None, epsilon=1e-20):
    """(fd, inner): the central difference of the total loss under xy +- h d_xy (P, 2) and Cartesian coefficients +- h d_cart (14, 2),
    and <grad, d> from probe_parameter_gradient of potential_gradient's probe gradient"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ab = aberration_cartesian(aberrations, wavelength) if cartesian is None else np.asarray(cartesian, dtype=np.float64)
    d_xy, d_cart = np.asarray(d_xy, dtype=np.float64), np.asarray(d_cart, dtype=np.float64)
    kw = dict(loss=loss, weight=weight, epsilon=epsilon)
    L = lambda s: probe_loss(nx, ny, dx, dy, wavelength, mrad, xy + s * d_xy, V, data, sigma, prop, cartesian=ab + s * d_cart, **kw)
    fd = (L(h) - L(-h)) / (2.0 * h)
    probes = np.fft.ifft2(probe_spectrum(nx, ny, dx, dy, wavelength, mrad, xy, cartesian=ab), axes=_AX)
    g0 = potential_gradient(probes, V, data, sigma, prop, **kw)[2]
    pos, cart, _ = probe_parameter_gradient(g0, nx, ny, dx, dy, wavelength, mrad, xy, cartesian=ab)
    return fd, float((pos * d_xy).sum() + (cart * d_cart).sum())


class Gradient:
    """MultisliceCalculator(gradient=Gradient(...)): run_gradient(data) returns dL/dV of the loss between the run's exit patterns
    and `data`.  loss: "amplitude", "intensity" or "poisson"; weight: (nx, ny) >= 0 in the detector's layout, or None; epsilon: the
    floor of |Psi|^2 in the amplitude and Poisson residuals; probe=True also returns dL/dpsi_0* per probe; positions=True also
    returns dL/dr_a per atom (GradientData.positions: the potential build backwards, section 4.32); probe_positions=True and
    aberrations=True also return dL/d(x_p, y_p) per scan position and dL/dC_nm, dL/dphi_nm of the probe-forming lens
    (GradientData.probe_position_gradient / .aberration_gradient: the probe recipe backwards, section 4.33)."""

    def __init__(self, loss="amplitude", weight=None, epsilon=1e-20, probe=False, positions=False, probe_positions=False, aberrations=False):
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
        self.probe_positions, self.aberrations = bool(probe_positions), bool(aberrations)

    @property
    def probe_params(self):
        """the run goes on through the probe recipe (msl_adjoint_probe_params)"""
        return self.probe_positions or self.aberrations

    @property
    def kind(self):
        return LOSSES[self.loss]

    def __repr__(self):
        return (f"Gradient(loss={self.loss!r}, weight={'None' if self.weight is None else self.weight.shape}, epsilon={self.epsilon:g}, "
                f"probe={self.probe}" + (", positions=True" if self.positions else "")
                + (", probe_positions=True" if self.probe_positions else "") + (", aberrations=True" if self.aberrations else "") + ")")

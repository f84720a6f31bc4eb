"""Finite projection: the part of every atom's 3D Kirkland potential that lies IN a slice.

Without it every potential of this package is an infinite projection: an atom drops into the one slice whose [lo, hi) holds its z
and leaves its whole projected form factor f_Z(k^2) there.  `MultisliceCalculator(projection=Projection(reach, nodes))`,
`projection="finite"` and `Potential(..., projection=...)` switch the device to the slab-integrated potential
(msl_set_projection, csrc/finite.h).  This module is its float64 NumPy definition, with no code shared with the engine path.

The model.  Kirkland's parameterisation is a 3D scattering factor f(q^2) = sum_j a_j / (q^2 + b_j) + c_j exp(-d_j q^2),
q^2 = k^2 + k_z^2.  The part of an atom's potential in the slab zeta = z - z_atom in [alpha, beta) has the in-plane transform

    F_Z(k; alpha, beta) = sum_j a_j / (2 kappa_j^2) [S(beta, kappa_j) - S(alpha, kappa_j)]
                          + c_j exp(-d_j k^2) 1/2 [erf(pi beta / sqrt d_j) - erf(pi alpha / sqrt d_j)],
    kappa_j = sqrt(k^2 + b_j),   S(zeta, kappa) = sgn(zeta) (1 - exp(-2 pi kappa |zeta|)),   S(+-inf, kappa) = +-1,

so that F_Z(k; -inf, +inf) = f_Z(k^2).  z is resolved on node planes: slabs are uniform, slab s = [e_s, e_s + dz) with
e_s = c_0 - dz/2 + s dz (c_s the slice coordinates), J nodes per slab at spacing h = dz / J, node n at e_0 + n h.  An atom at z has
g = (z - e_0) / h, n0 = floor(g), w = g - n0 and becomes two partial atoms, weight 1 - w on node n0 and w on n0 + 1.  Node n gives
slab s, m = n - s J in [-R J, (R + 1) J), the table F_Z(k; -m h, -m h + dz); in the lowest slab it reaches alpha = -inf and in the
highest beta = +inf (tail folding), so truncation moves charge by at most R dz and never loses it.  An atom counts iff it counts in
the infinite projection (lo[0] <= z < hi[nz-1]); what it would give to slabs outside the stack is dropped.
"""
from __future__ import annotations

import math

import numpy as np

from .potentials import loadKirkland, slice_edges

MAX_REACH_SLICES, MAX_NODES = 32, 16       # include/mslice.h: msl_set_projection


class Projection:
    """MultisliceCalculator(projection=Projection(reach, nodes)): `reach` in Angstrom -- an atom's potential is spread over the slices
    within R = ceil(reach / dz) of its own, the tails beyond folded into the outermost two -- and `nodes` planes per slice on which
    z is resolved (the z error of an atom is at most dz / nodes)."""

    def __init__(self, reach=2.0, nodes=4):
        if isinstance(reach, bool) or not isinstance(reach, (int, float, np.integer, np.floating)) or not math.isfinite(reach) or not reach > 0:
            raise ValueError(f"Projection: reach must be a positive length in Angstrom, got {reach!r}")
        if isinstance(nodes, bool) or not isinstance(nodes, (int, np.integer)) or not 1 <= int(nodes) <= MAX_NODES:
            raise ValueError(f"Projection: nodes must be an integer in 1..{MAX_NODES}, got {nodes!r}")
        self.reach, self.nodes = float(reach), int(nodes)

    def reach_slices(self, dz):
        """R = ceil(reach / dz) for slices dz thick; a ValueError beyond the engine's 32"""
        if not dz > 0:
            raise ValueError(f"projection: the slice thickness must be positive, got {dz!r}")
        R = max(1, int(math.ceil(self.reach / float(dz) - 1e-9)))
        if R > MAX_REACH_SLICES:
            raise ValueError(f"projection: a reach of {self.reach:g} A is {R} slices of {dz:g} A, more than {MAX_REACH_SLICES}: use thicker "
                             "slices or a shorter reach")
        return R

    def __repr__(self):
        return f"Projection(reach={self.reach:g}, nodes={self.nodes})"


def as_projection(value, what="projection"):
    """None / "infinite" -> None (off); "finite" -> Projection(); a Projection stays"""
    if value is None or (isinstance(value, str) and value == "infinite"):
        return None
    if isinstance(value, str) and value == "finite":
        return Projection()
    if isinstance(value, Projection):
        return value
    raise ValueError(f"{what}: expected a Projection object, 'finite', 'infinite' or None, got {value!r}")


def _S(zeta, kappa):
    if np.isinf(zeta):
        return np.sign(zeta) * np.ones_like(kappa)
    return np.sign(zeta) * -np.expm1(-2.0 * np.pi * kappa * abs(zeta))


def finite_form_factor(Z, k2, alpha, beta):
    """F_Z(k; alpha, beta) on an array of k^2 (float64); alpha, beta may be -inf / +inf"""
    from scipy.special import erf
    k2 = np.asarray(k2, dtype=np.float64)
    out = np.zeros_like(k2)
    for a, b, c, d in loadKirkland()[int(Z) - 1]:
        kap2 = k2 + b
        kap = np.sqrt(kap2)
        out = out + a / (2.0 * kap2) * (_S(beta, kap) - _S(alpha, kap))
        g = np.pi / np.sqrt(d)
        out = out + c * np.exp(-d * k2) * 0.5 * (erf(g * beta) - erf(g * alpha))
    return out


def _slab(m, R, J, dz):
    """(alpha, beta) of channel m of a node, with the tails folded"""
    h = dz / J
    alpha = -np.inf if m >= R * J else -m * h
    beta = np.inf if m < -(R - 1) * J else -m * h + dz
    return alpha, beta


def channel_tables(species, nx, ny, dx, dy, dz, reach_slices, nodes):
    """(len(species) * (2 R + 1) * J, nx, ny) float64: the tables of the device (MSL_BUF_FORMFACTOR_FINITE), species-major, then
    m = -R J .. (R + 1) J - 1"""
    R, J = int(reach_slices), int(nodes)
    kxs, kys = np.fft.fftfreq(nx, d=dx), np.fft.fftfreq(ny, d=dy)
    k2 = kxs[:, None] ** 2 + kys[None, :] ** 2
    out = [finite_form_factor(Z, k2, *_slab(m, R, J, dz)) for Z in species for m in range(-R * J, (R + 1) * J)]
    return np.stack(out)


def _grid(xs, ys, zs, slice_axis):
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs, ys, zs))
    axes = [0, 1, 2]
    axes.remove(slice_axis)
    coords = [xs, ys, zs][slice_axis]
    dz = coords[1] - coords[0] if len(coords) > 1 else 0.5
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    kxs, kys = np.fft.fftfreq(len(xs), d=dx), np.fft.fftfreq(len(ys), d=dy)
    return coords, dz, dx, dy, kxs, kys, axes


def finite_potential(xs, ys, zs, positions, Z, reach_slices, nodes, slice_axis=2):
    """V (nx, ny, n_slices) float64 of the finite projection with reach R = reach_slices and J = nodes, from the model of the module
    docstring: partial atoms on nodes, 2 R + 1 slabs per node, tails folded, contributions outside the stack dropped."""
    R, J = int(reach_slices), int(nodes)
    coords, dz, dx, dy, kxs, kys, (ax1, ax2) = _grid(xs, ys, zs, slice_axis)
    nz = len(coords)
    lo, hi = slice_edges(coords)
    e0, h = coords[0] - dz / 2, dz / J
    k2 = kxs[:, None] ** 2 + kys[None, :] ** 2
    positions, Z = np.asarray(positions, dtype=np.float64), np.asarray(Z)
    recip = np.zeros((nz, len(kxs), len(kys)), dtype=np.complex128)
    nodes_of = {}                                   # (Z, node) -> [(weight, x, y)]
    for (r, z) in zip(positions, Z):
        zc = r[slice_axis]
        if not (lo[0] <= zc < hi[-1]):
            continue
        g = (zc - e0) / h
        n0 = math.floor(g)
        w = g - n0
        nodes_of.setdefault((int(z), n0), []).append((1.0 - w, r[ax1], r[ax2]))
        if w > 0.0:
            nodes_of.setdefault((int(z), n0 + 1), []).append((w, r[ax1], r[ax2]))
    tables = {}
    for (z, n), rows in nodes_of.items():
        wt, px, py = (np.array(v) for v in zip(*rows))
        sf = (np.exp(-2j * np.pi * np.outer(kxs, px)) * wt) @ np.exp(-2j * np.pi * np.outer(py, kys))
        for s in range(nz):
            m = n - s * J
            if -R * J <= m < (R + 1) * J:
                if (z, m) not in tables:
                    tables[z, m] = finite_form_factor(z, k2, *_slab(m, R, J, dz))
                recip[s] += tables[z, m] * sf
    v = np.fft.ifft2(recip, axes=(1, 2)).real / (dx ** 2 * dy ** 2)
    return np.ascontiguousarray(np.moveaxis(v, 0, 2))


def exact_slab_potential(xs, ys, zs, positions, Z, slice_axis=2):
    """V (nx, ny, n_slices) float64 with every atom at its true z: slab s takes F_Z(k; e_s - z, e_s + dz - z) of every atom that
    counts -- no nodes, no truncation, no folding.  What finite_potential converges to as nodes and reach grow."""
    coords, dz, dx, dy, kxs, kys, (ax1, ax2) = _grid(xs, ys, zs, slice_axis)
    nz = len(coords)
    lo, hi = slice_edges(coords)
    e0 = coords[0] - dz / 2
    k2 = kxs[:, None] ** 2 + kys[None, :] ** 2
    recip = np.zeros((nz, len(kxs), len(kys)), dtype=np.complex128)
    for (r, z) in zip(np.asarray(positions, dtype=np.float64), np.asarray(Z)):
        zc = r[slice_axis]
        if not (lo[0] <= zc < hi[-1]):
            continue
        phase = np.exp(-2j * np.pi * kxs * r[ax1])[:, None] * np.exp(-2j * np.pi * kys * r[ax2])[None, :]
        for s in range(nz):
            a = e0 + s * dz - zc
            recip[s] += finite_form_factor(int(z), k2, a, a + dz) * phase
    v = np.fft.ifft2(recip, axes=(1, 2)).real / (dx ** 2 * dy ** 2)
    return np.ascontiguousarray(np.moveaxis(v, 0, 2))

"""Element maps: the channelling-weighted ionisation signal per element, what an EDX map or a core-loss EELS map records.

In the local approximation the probability that the probe ionises an atom is the probe intensity inside the specimen integrated
against a short-ranged interaction potential centred on that atom.  A channel e is an element, a 2D Gaussian of rms width w_e
(Angstrom) in the place of that potential and a cross-section c_e (Angstrom^2).  For frame t, slice s, with A the atoms of the
element that the potential build assigns to slice s (slice_edges: lo[s] <= z < hi[s], the rule of potentials.py and of
msl_build_potential, no second one),

    W^_e,s(k) = c_e exp(-2 pi^2 w_e^2 |k|^2) sum_{i in A} exp(-2 pi i k r_i)          on the fftfreq grid
    W_e,s(r)  = real(ifft2(W^)) / (dx dy)                                            the periodised Gaussian, sum_r W dx dy = c_e |A|
    I[p, e, s] = (1/T) sum_t sum_r |psi_p,t,s(r)|^2 W_e,s,t(r) / sum_r |psi_p,0(r)|^2

psi_p,t,s the wave arriving at slice s, before t_s (the wave tds.tds_signal uses).  I is the ionisation probability per incident
electron in slice s; for a plane wave on the first slice it is n_e c_e / (cell area) exactly.  The sum over s is the signal of a
map, the partial sums are the beam-channelling curve.

The approximation, plainly: it is local -- one Gaussian per channel instead of a tabulated, energy- and angle-dependent transition
potential, so delocalisation is a single width and the detector geometry is not in it.  The elastic wave is not depleted by the
ionisation, and the ionised (and the inelastically scattered) electrons are not followed: the signal is generated, not detected.

The device builds the same weights and sums itself (csrc/ionization.h behind msl_set_ionization).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_IONIZATION_CHANNELS = 8


def _element(element):
    """atomic number of an element given as a number or a name, the way FrozenPhonons resolves the keys of `sigma`"""
    from .potentials import getZfromElementName
    if isinstance(element, str):
        try:
            Z = getZfromElementName(element)
        except ValueError:
            raise ValueError(f"Ionization: unknown element name {element!r}") from None
    elif isinstance(element, (int, np.integer)) and not isinstance(element, bool):
        Z = int(element)
    else:
        raise ValueError(f"Ionization: element must be an atomic number or an element name, got {element!r}")
    if not 1 <= Z <= 103:
        raise ValueError(f"Ionization: atomic number {Z} outside 1..103")
    return Z


@dataclass(frozen=True, init=False)
class Ionization:
    """One channel of MultisliceCalculator(ionization=[...]): element (atomic number or name), width > 0 the rms width in Angstrom
    of the 2D Gaussian, cross_section >= 0 in Angstrom^2, name (default: the element symbol).  Two channels may name one element with
    different widths: two edges."""
    Z: int
    width: float
    cross_section: float
    name: str

    def __init__(self, element, width, cross_section=1.0, name=None):
        Z = _element(element)
        try:
            w, c = float(width), float(cross_section)
        except (TypeError, ValueError):
            raise ValueError(f"Ionization: width and cross_section must be numbers, got {width!r}, {cross_section!r}") from None
        if not (np.isfinite(w) and w > 0.0):
            raise ValueError(f"Ionization: width must be a finite number > 0 (Angstrom), got {width!r}")
        if not (np.isfinite(c) and c >= 0.0):
            raise ValueError(f"Ionization: cross_section must be a finite number >= 0 (Angstrom^2), got {cross_section!r}")
        object.__setattr__(self, "Z", Z)
        object.__setattr__(self, "width", w)
        object.__setattr__(self, "cross_section", c)
        from .potentials import _ELEMENTS
        object.__setattr__(self, "name", _ELEMENTS[Z - 1] if name is None else str(name))


def check_ionization(channels):
    """the `ionization` argument of MultisliceCalculator -> a list of 1 to 8 Ionization objects"""
    if isinstance(channels, Ionization):
        channels = [channels]
    try:
        channels = list(channels)
    except TypeError:
        raise ValueError(f"ionization: expected a list of Ionization objects, got {channels!r}") from None
    for ch in channels:
        if not isinstance(ch, Ionization):
            raise ValueError(f"ionization: expected Ionization objects, got {ch!r}")
    if not 1 <= len(channels) <= MAX_IONIZATION_CHANNELS:
        raise ValueError(f"ionization: 1 to {MAX_IONIZATION_CHANNELS} channels, got {len(channels)}")
    return channels


def ionization_weights(channels, xs, ys, slice_coords, positions, atomic_numbers, slice_axis=2):
    """W (E, nz, nx, ny) float64 of one frame: channels a list of Ionization, xs / ys the pixel coordinates of the two in-plane axes,
    slice_coords those of the slice axis (their edges: potentials.slice_edges), positions (n, 3), atomic_numbers (n,)"""
    from .potentials import slice_edges
    channels = check_ionization(channels)
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    Z = np.asarray(atomic_numbers).reshape(-1)
    if len(Z) != len(pos):
        raise ValueError(f"ionization_weights: {len(pos)} positions, {len(Z)} atomic numbers")
    nx, ny = len(xs), len(ys)
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    lo, hi = slice_edges(np.asarray(slice_coords, dtype=np.float64))
    ax1, ax2 = [a for a in range(3) if a != slice_axis]
    kx, ky = np.fft.fftfreq(nx, dx), np.fft.fftfreq(ny, dy)
    q2 = kx[:, None] ** 2 + ky[None, :] ** 2
    W = np.zeros((len(channels), len(lo), nx, ny), dtype=np.float64)
    for e, ch in enumerate(channels):
        sel = pos[Z == ch.Z]
        damp = ch.cross_section * np.exp(-2.0 * np.pi ** 2 * ch.width ** 2 * q2)
        for s in range(len(lo)):
            m = (sel[:, slice_axis] >= lo[s]) & (sel[:, slice_axis] < hi[s])
            if not m.any():
                continue
            S = np.exp(-2j * np.pi * np.outer(kx, sel[m, ax1])) @ np.exp(-2j * np.pi * np.outer(sel[m, ax2], ky))
            W[e, s] = np.fft.ifft2(damp * S).real / (dx * dy)
    return W


def ionization_signal(psi0, transmission, weights, propagator):
    """The float64 slice loop, shaped like tds.tds_signal: psi0 (P, nx, ny) incident waves, transmission (nz, nx, ny) complex,
    weights (E, nz, nx, ny) (ionization_weights), propagator (nx, ny) on the fftfreq grid (the Fresnel factor of one slice;
    tilt.tilted_propagator) -> (I (P, E, nz) per incident electron, exit waves (P, nx, ny))."""
    psi = np.array(psi0, dtype=np.complex128)
    if psi.ndim == 2:
        psi = psi[None]
    t = np.asarray(transmission)
    w = np.asarray(weights, dtype=np.float64)
    if t.ndim != 3 or t.shape[1:] != psi.shape[1:]:
        raise ValueError(f"ionization_signal: transmission {t.shape} does not match the waves {psi.shape}: expected (nz, nx, ny)")
    if w.ndim != 4 or w.shape[1:] != t.shape:
        raise ValueError(f"ionization_signal: weights {w.shape} do not match the transmission {t.shape}: expected (E, nz, nx, ny)")
    nz = t.shape[0]
    n0 = (np.abs(psi) ** 2).sum(axis=(1, 2))
    I = np.zeros((psi.shape[0], w.shape[0], nz), dtype=np.float64)
    for s in range(nz):
        I[:, :, s] = np.einsum("pxy,exy->pe", np.abs(psi) ** 2, w[:, s]) / n0[:, None]
        psi = t[s][None] * psi
        if s < nz - 1:
            psi = np.fft.ifft2(np.asarray(propagator)[None] * np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))
    return I, psi

"""Absorptive potential: the thermal average of the elastic wave in ONE pass through a complex potential, and the input type
that carries it.

The frozen-phonon ensemble (thermal.FrozenPhonons) averages 20-60 full slice loops.  Where only the elastic signal is wanted --
HRTEM images, CBED / PACBED discs, bright field, ABF, DPC -- the classical alternative is the mean transmission function of every
slice: for independent Gaussian displacements of rms width u per axis, and to second order in the fluctuation of sigma V,

    <exp(i sigma V_s)>  ~  t_s = exp(i sigma Vbar_s - sigma^2 Omega_s),      Omega_s = 1/2 Var V_s

Vbar the Debye-Waller-smeared mean potential, Omega the absorption that thermal diffuse scattering takes out of the elastic channel
(Hall & Hirsch 1965, for atoms projected into one slice).  Mean and variance of independent atoms superpose linearly, so both are the
structure-factor sum of the ordinary potential build with other per-species tables.  This file is the definition, in NumPy and
float64, on the simulation grid -- with its band limit and the reference's 1 / (dx^2 dy^2) normalisation (potentials.py:336-342) -- so
that it agrees with the engine's own frozen-phonon runs:

    D     = exp(-2 pi^2 u^2 q^2)
    V1    = real(ifft2(f))     / (dx^2 dy^2)            one atom as the engine rasterises it
    Vbar1 = real(ifft2(f D))   / (dx^2 dy^2)            its thermal mean
    Om1   = 1/2 (real(ifft2(D fft2(V1^2))) - Vbar1^2)   1/2 Var V1 under the Gaussian
    g     = real(fft2(Om1)) dx^2 dy^2                   the "absorptive form factor", real and even

The device builds the same tables itself (csrc/absorptive.h behind msl_set_absorption).

The model is the classical weak-fluctuation one: its error is third order in sigma V of ONE atom in one slice.  For carbon at 100 keV
and 0.1 A sampling max |t - <t>| is 1e-3; for gold at the same sampling, where sigma V reaches 7.5 rad at the atom centre, it is
0.56 -- use the ensemble there.

The TDS signal that this absorption feeds to a detector (HAADF from the same pass) is tds.py.

Not built: per-atom widths inside one element, anisotropic u, the exact per-atom mean transmission in place of the second cumulant,
a fused one-pass structure factor for both tables.
"""
from __future__ import annotations

import numpy as np

from .potentials import _ELEMENTS, atomic_numbers_of
from .thermal import FrozenPhonons, per_atom_sigma


def debye_waller(q2, u):
    """D = exp(-2 pi^2 u^2 q^2): the Fourier transform of the Gaussian of rms width u per axis (u = 0: exactly 1)"""
    return np.exp(-2.0 * np.pi ** 2 * float(u) ** 2 * np.asarray(q2, dtype=np.float64))


def absorptive_tables(f, q2, u, dx, dy, complex_g=False):
    """(f D, g) of one species: f its form-factor table on the fftfreq grid, q2 = kx^2 + ky^2 there, u its rms width per axis.
    u = 0 is no vibration: f D is f bit for bit and g is zero.  complex_g: g before its real part is taken (its imaginary part is
    rounding noise: Om1 is real and even)."""
    f = np.asarray(f, dtype=np.float64)
    cell = float(dx) ** 2 * float(dy) ** 2
    D = debye_waller(q2, u)
    fD = f * D
    if float(u) == 0.0:
        return fD, np.zeros(f.shape, dtype=np.complex128 if complex_g else np.float64)
    V1 = np.fft.ifft2(f).real / cell
    Vbar1 = np.fft.ifft2(fD).real / cell
    Om1 = 0.5 * (np.fft.ifft2(D * np.fft.fft2(V1 ** 2)).real - Vbar1 ** 2)
    g = np.fft.fft2(Om1) * cell
    return fD, (g if complex_g else g.real)


def absorptive_transmission(Vbar, Omega, sigma_e):
    """t = exp(i sigma Vbar - sigma^2 Omega), sigma_e the interaction constant"""
    return np.exp(1j * sigma_e * np.asarray(Vbar, dtype=np.float64) - sigma_e ** 2 * np.asarray(Omega, dtype=np.float64))


def mean_transmission_exact(f, q2, u, dx, dy, sigma_e):
    """<exp(i sigma V1)> of ONE atom over its Gaussian displacement, exactly: the convolution of exp(i sigma V1) with the Gaussian"""
    cell = float(dx) ** 2 * float(dy) ** 2
    V1 = np.fft.ifft2(np.asarray(f, dtype=np.float64)).real / cell
    return np.fft.ifft2(debye_waller(q2, u) * np.fft.fft2(np.exp(1j * sigma_e * V1)))


class AbsorptivePotential:
    """One structure with the thermal vibration in its potential, as an input of MultisliceCalculator.setup() in place of a
    Trajectory: a single frame whose transmission functions are exp(i sigma Vbar - sigma^2 Omega).  `positions` (n_atoms, 3) is the
    structure, `sigma` the rms displacement along each Cartesian axis in Angstrom as in FrozenPhonons (per_atom_sigma: a float, a
    mapping by species, or one value per atom; sigma_from_B turns Debye-Waller factors into it) -- it must come out as ONE value per
    element.  absorption=False keeps the Debye-Waller damping and leaves Omega out."""

    def __init__(self, atom_types, positions, box_matrix, sigma, absorption=True, timestep=1.0):
        self.atom_types = np.asarray(atom_types)
        base = np.ascontiguousarray(positions, dtype=np.float64)
        self.box_matrix = np.asarray(box_matrix)
        self.timestep = timestep
        self.absorption = bool(absorption)
        if base.ndim != 2 or base.shape[1] != 3:
            raise ValueError(f"positions must be (atoms, 3), got {base.shape}")
        if self.atom_types.ndim != 1:
            raise ValueError(f"atom_types must be 1D, got {self.atom_types.ndim}D")
        if self.box_matrix.shape != (3, 3):
            raise ValueError(f"box_matrix must be (3, 3), got {self.box_matrix.shape}")
        if base.shape[0] != len(self.atom_types):
            raise ValueError(f"Atom count mismatch: {base.shape[0]}, {len(self.atom_types)}")
        if not np.all(np.isfinite(base)):
            raise ValueError("positions must be finite")
        self.base_positions = base
        self.positions = base[None]                 # (1, n_atoms, 3): the one frame, where a Trajectory keeps its frames
        self.sigma = per_atom_sigma(sigma, self.atom_types)
        Z = atomic_numbers_of(self.atom_types)
        if np.any(Z < 1) or np.any(Z > 103):
            raise ValueError("atomic numbers must be in 1..103")
        self.u_by_Z = np.zeros(103, dtype=np.float64)           # the argument of msl_set_absorption
        for z in np.unique(Z):
            widths = np.unique(self.sigma[Z == z])
            if widths.size != 1:
                raise ValueError(f"sigma: element {_ELEMENTS[int(z) - 1]} (Z = {int(z)}) has {widths.size} different widths; the absorptive "
                                 "potential takes one width per element (per-atom widths inside one element are not built)")
            self.u_by_Z[int(z) - 1] = widths[0]

    @classmethod
    def from_trajectory(cls, trajectory, sigma, frame=0, absorption=True):
        """the structure is frame `frame` of a Trajectory (its box, species and timestep are kept)"""
        if not 0 <= int(frame) < trajectory.n_frames:
            raise ValueError(f"frame {frame} outside [0, {trajectory.n_frames})")
        return cls(trajectory.atom_types, trajectory.positions[int(frame)], trajectory.box_matrix, sigma, absorption=absorption,
                   timestep=trajectory.timestep)

    @property
    def n_frames(self) -> int:
        return 1

    @property
    def n_atoms(self) -> int:
        return len(self.atom_types)

    @property
    def box_tilts(self) -> np.ndarray:
        return np.array([self.box_matrix[0, 1], self.box_matrix[0, 2], self.box_matrix[1, 2]])

    def frozen_phonons(self, n_configs, seed=0):
        """the ensemble this potential is the average of"""
        return FrozenPhonons(self.atom_types, self.base_positions, self.box_matrix, self.sigma, n_configs, seed=seed, timestep=self.timestep)

"""Frozen phonons (Einstein model): the definition of a configuration, and the input type that carries it.

A configuration is a pure function of (seed, configuration index, atom index): every atom of the base structure is displaced by
an independent Gaussian of its own width, drawn from the counter-based generator Philox-4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11; the Random123 library).  This file is the definition, in NumPy and float64 on the host; the
device generates the same numbers itself (csrc/thermal.h: thermal_positions_kernel behind msl_build_thermal), so that no
configuration is ever stored or copied, and `FrozenPhonons.configuration(k)` / `Engine.thermal_positions(seed, k)` say what it used.

    counter of atom i, configuration c:  (i, c & 0xffffffff, c >> 32, 0)         key: (seed & 0xffffffff, seed >> 32)
    x0..x3 = philox4x32_10(counter, key)       u_j = (x_j + 0.5) * 2^-32   in (0, 1)
    g_x = sqrt(-2 ln u0) cos(2 pi u1)   g_y = sqrt(-2 ln u0) sin(2 pi u1)   g_z = sqrt(-2 ln u2) cos(2 pi u3)
    position = base + sigma * (g_x, g_y, g_z)

g_x, g_y, g_z belong to columns 0, 1, 2 of the positions array, whatever the slice axis is.  Nothing is wrapped or clipped: the
slice rule of the potential treats a configuration exactly as it treats a trajectory frame, so an atom pushed out of the stack
along the slice axis is dropped (leave a few sigma of vacuum at the entrance and exit surfaces) and the in-plane axes are periodic
anyway.

Not built: anisotropic or per-axis widths, wrapping at the surfaces.  Correlated (phonon-mode) displacements are phonons.PhononModes.
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np

from .trajectory import Trajectory

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57           # the multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85           # the Weyl constants the key advances by every round
_MASK = np.uint64(0xFFFFFFFF)
_U64_MAX = (1 << 64) - 1


def philox4x32_10(counter, key):
    """Philox-4x32 with 10 rounds: counter (..., 4) uint32, key (2,) uint32 -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32).reshape(-1)
    if c.shape[-1] != 4 or k.shape != (2,):
        raise ValueError(f"philox4x32_10: counter (..., 4) and key (2,) required, got {c.shape} and {k.shape}")
    c0, c1, c2, c3 = (c[..., j].astype(np.uint64) for j in range(4))
    k0, k1 = int(k[0]), int(k[1])
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0                  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(x):
    """uint32 -> float64 in (0, 1): (x + 0.5) * 2^-32, exact in float64"""
    return (np.asarray(x, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def _u64(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= _U64_MAX:
        raise ValueError(f"{name} must be a non-negative 64-bit integer, got {v!r}")
    return int(v)


def normals(seed, config, n_atoms):
    """(n_atoms, 3) float64: the standard normals (g_x, g_y, g_z) of every atom of configuration `config`"""
    seed, config = _u64("seed", seed), _u64("config", config)
    n = int(n_atoms)
    if not 0 <= n < 2 ** 31:
        raise ValueError(f"n_atoms must be in [0, 2^31), got {n_atoms}")
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    ctr[:, 1] = config & 0xFFFFFFFF
    ctr[:, 2] = config >> 32
    u = uniforms(philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)))
    r01 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r23 = np.sqrt(-2.0 * np.log(u[:, 2]))
    a01 = 2.0 * np.pi * u[:, 1]
    return np.stack([r01 * np.cos(a01), r01 * np.sin(a01), r23 * np.cos(2.0 * np.pi * u[:, 3])], axis=1)


def displaced(base, sigma, seed, config):
    """base (n, 3) + sigma (n,) [:, None] * normals(seed, config, n): one configuration, not wrapped, not clipped"""
    base = np.asarray(base, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    if base.ndim != 2 or base.shape[1] != 3:
        raise ValueError(f"base must be (atoms, 3), got {base.shape}")
    if sigma.shape != (base.shape[0],):
        raise ValueError(f"sigma must be ({base.shape[0]},), got {sigma.shape}")
    return base + sigma[:, None] * normals(seed, config, base.shape[0])


def sigma_from_B(B):
    """rms displacement along each Cartesian axis (Angstrom) from the Debye-Waller factor B = 8 pi^2 <u_x^2> (Angstrom^2)"""
    return np.sqrt(np.asarray(B, dtype=np.float64) / (8.0 * np.pi ** 2))


def _atomic_number(species):
    from .potentials import getZfromElementName
    if isinstance(species, str):
        try:
            return getZfromElementName(species)
        except ValueError:
            raise ValueError(f"sigma: unknown element name {species!r}") from None
    return int(species)


def per_atom_sigma(sigma, atom_types):
    """the `sigma` argument of FrozenPhonons -> (n_atoms,) float64: a float, a mapping from atomic number or element name to a
    float (every species present must be named), or one value per atom; every value finite and >= 0"""
    n = len(atom_types)
    if isinstance(sigma, Mapping):
        by_Z = {_atomic_number(key): float(v) for key, v in sigma.items()}
        Z = np.asarray([_atomic_number(t) for t in atom_types], dtype=np.int64)
        missing = sorted(set(Z.tolist()) - set(by_Z))
        if missing:
            raise ValueError(f"sigma names no width for the species {missing} (atomic numbers) of the structure")
        out = np.asarray([by_Z[z] for z in Z.tolist()], dtype=np.float64).reshape(n)
    else:
        out = np.asarray(sigma, dtype=np.float64)
        if out.ndim == 0:
            out = np.full(n, float(out))
        elif out.shape != (n,):
            raise ValueError(f"sigma must be a float, a mapping by species or ({n},) values, got shape {out.shape}")
        else:
            out = out.copy()
    if not np.all(np.isfinite(out)) or np.any(out < 0):
        raise ValueError("sigma: every width must be finite and >= 0")
    return out


class FrozenPhonons:
    """`n_configs` Einstein-model configurations of one structure, as an input of MultisliceCalculator.setup(): what a Trajectory
    of n_configs frames is, without the frames.  `positions` (n_atoms, 3) is the base structure, `sigma` the rms displacement
    along each Cartesian axis in Angstrom (per_atom_sigma: a float, a mapping by species, or one value per atom; sigma_from_B turns
    Debye-Waller factors into it), `seed` a non-negative 64-bit integer.  configuration(k) is the definition of frame k; the
    device generates the same positions itself, so nothing per configuration is stored or copied."""

    def __init__(self, atom_types, positions, box_matrix, sigma, n_configs, seed=0, timestep=1.0):
        self.atom_types = np.asarray(atom_types)
        self.positions = np.ascontiguousarray(positions, dtype=np.float64)
        self.box_matrix = np.asarray(box_matrix)
        self.timestep = timestep
        # the messages of Trajectory._validate_shapes where they apply (trajectory.py)
        if self.positions.ndim != 2 or self.positions.shape[1] != 3:
            raise ValueError(f"positions must be (atoms, 3), got {self.positions.shape}")
        if self.atom_types.ndim != 1:
            raise ValueError(f"atom_types must be 1D, got {self.atom_types.ndim}D")
        if self.box_matrix.shape != (3, 3):
            raise ValueError(f"box_matrix must be (3, 3), got {self.box_matrix.shape}")
        if self.positions.shape[0] != len(self.atom_types):
            raise ValueError(f"Atom count mismatch: {self.positions.shape[0]}, {len(self.atom_types)}")
        if not self.n_atoms < 2 ** 31:
            raise ValueError("n_atoms must be below 2^31")
        if not np.all(np.isfinite(self.positions)):
            raise ValueError("positions must be finite")
        if isinstance(n_configs, (bool, np.bool_)) or not isinstance(n_configs, (int, np.integer)) or int(n_configs) < 1:
            raise ValueError(f"n_configs must be a positive integer, got {n_configs!r}")
        self.n_configs = int(n_configs)
        self.seed = _u64("seed", seed)
        self.sigma = per_atom_sigma(sigma, self.atom_types)

    @classmethod
    def from_trajectory(cls, trajectory, sigma, n_configs, seed=0, frame=0):
        """the base structure is frame `frame` of a Trajectory (its box, species and timestep are kept)"""
        if not 0 <= int(frame) < trajectory.n_frames:
            raise ValueError(f"frame {frame} outside [0, {trajectory.n_frames})")
        return cls(trajectory.atom_types, trajectory.positions[int(frame)], trajectory.box_matrix, sigma, n_configs, seed=seed,
                   timestep=trajectory.timestep)

    @property
    def n_frames(self) -> int:
        return self.n_configs

    @property
    def n_atoms(self) -> int:
        return len(self.atom_types)

    @property
    def box_tilts(self) -> np.ndarray:
        return np.array([self.box_matrix[0, 1], self.box_matrix[0, 2], self.box_matrix[1, 2]])

    def configuration(self, k):
        """(n_atoms, 3) float64: configuration k >= 0 (any index: n_configs only says how many a run takes)"""
        return displaced(self.positions, self.sigma, self.seed, _u64("configuration index", k))

    def absorptive(self, absorption=True):
        """the absorptive.AbsorptivePotential of the same structure and widths: the ensemble's elastic average in one pass"""
        from .absorptive import AbsorptivePotential
        return AbsorptivePotential(self.atom_types, self.positions, self.box_matrix, self.sigma, absorption=absorption, timestep=self.timestep)

    def to_trajectory(self, configs=None):
        """The configurations (None: 0 .. n_configs - 1) as a Trajectory on the host, 24 B x n_atoms each: for tests and small
        cases."""
        ks = range(self.n_configs) if configs is None else list(configs)
        pos = np.stack([self.configuration(k) for k in ks]) if len(ks) else np.zeros((0, self.n_atoms, 3))
        return Trajectory(atom_types=self.atom_types, positions=pos, velocities=np.zeros_like(pos), box_matrix=self.box_matrix,
                          timestep=self.timestep)

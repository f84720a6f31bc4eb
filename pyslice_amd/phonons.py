"""Phonon modes: the definition of a frame synthesised from a set of lattice-dynamics modes, and the input type that carries it.

A phonon model is a list of M modes, each with a wave vector q_m (Cartesian, cycles / Angstrom, in columns 0, 1, 2 like the
positions, whatever the slice axis is), a frequency nu_m (cycles per unit of `timestep`: the unit of TACAWData.frequencies) and a
complex displacement vector W[m, b, :] (Angstrom per unit normal coordinate) for every basis atom b; atom i of the structure is a
copy of basis atom b_i at the base position r_i.  A frame is a pure function of (seed, frame index): this file is the definition, in
NumPy and float64 on the host; the device computes the same numbers itself (csrc/phonons.h: mode_coefficients_kernel and
mode_positions_kernel behind msl_build_modes), so that no frame is ever stored or copied, and `PhononModes.configuration(c)` /
`Engine.mode_positions(seed, c)` say what it used.

    normal coordinate of mode m under draw index k:
        counter (m, k & 0xffffffff, k >> 32, 1)    key (seed & 0xffffffff, seed >> 32)     (thermal.py: word 3 = 0 is the Einstein stream)
        x0, x1 = philox4x32_10(counter, key)[:2]   u_j = (x_j + 0.5) * 2^-32
        g = sqrt(-ln u0) * exp(2 pi i u1)           a complex Gaussian with <|g|^2> = 1
    frame c:   dynamic (a time-coherent record):   k = 0 for every frame,  theta = tau_m * c,   tau_m = nu_m * timestep (rounded once)
               snapshots (dynamic=False):          k = c,                  theta = 0
    frac(y) = y - rint(y)
    C[c, m] = g_m(k) * exp(-2 pi i frac(theta))
    x       = (q0 r0 + q1 r1) + q2 r2               every product and every sum rounded separately
    E       = exp(2 pi i frac(x))
    u_i(c)  = sum_m Re[ (C[c, m] E) W[m, b_i, :] ]  summed in mode order
    position = r_i + u_i(c)

With independent normal coordinates <g g*> = 1, <g g> = 0, so every Cartesian component of every atom has the variance

    <u_{i alpha}^2> = 1/2 sum_m |W[m, b_i, alpha]|^2

in both frame rules (over seeds for a dynamic record, over frames for snapshots).  A dynamic record moves every mode as
exp(2 pi i (q.r - nu t)): a wave travelling along +q.  To first order the exit wave carries that factor and its conjugate, so with
the transforms of TACAWData (numpy.fft in time and space) the intensity of the mode sits at frequency -nu around G + q and at +nu
around G - q of every Bragg spot G.

Nothing is wrapped or clipped: the slice rule of the potential treats a frame exactly as it treats a trajectory frame (thermal.py).

Not built: Einstein widths added on top of the modes, anharmonic or damped modes, per-mode occupations that change over time,
reading the phonon files of other codes, interpolating force constants.
"""
from __future__ import annotations

import numpy as np

from .thermal import _u64, philox4x32_10, uniforms
from .trajectory import Trajectory

# CODATA 2018 (exact since the 2019 SI), and the atomic mass constant
HBAR_J_S = 1.054571817e-34
K_B_J_PER_K = 1.380649e-23
AMU_KG = 1.66053906660e-27


def frac(y):
    """y - rint(y): the phase in cycles brought to [-1/2, 1/2]; the subtraction is exact in float64"""
    y = np.asarray(y, dtype=np.float64)
    return y - np.rint(y)


def normal_coordinates(seed, draw, n_modes):
    """(n_modes,) complex128: the random normal coordinate g of every mode under draw index `draw`"""
    seed, draw = _u64("seed", seed), _u64("draw index", draw)
    M = int(n_modes)
    if not 0 <= M < 2 ** 31:
        raise ValueError(f"n_modes must be in [0, 2^31), got {n_modes}")
    ctr = np.zeros((M, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(M, dtype=np.uint32)
    ctr[:, 1] = draw & 0xFFFFFFFF
    ctr[:, 2] = draw >> 32
    ctr[:, 3] = 1
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u0, u1 = uniforms(x[:, 0]), uniforms(x[:, 1])
    a = 2.0 * np.pi * u1
    return np.sqrt(-np.log(u0)) * (np.cos(a) + 1j * np.sin(a))


def mode_coefficients(tau, seed, frames, dynamic=True):
    """(len(frames), M) complex128: C[c, m] of the frames `frames` (any non-negative indices) for the per-mode phase advances
    tau (M,) = nu * timestep in cycles per frame"""
    tau = np.asarray(tau, dtype=np.float64)
    if tau.ndim != 1:
        raise ValueError(f"tau must be (modes,), got {tau.shape}")
    frames = [_u64("frame index", c) for c in frames]
    out = np.empty((len(frames), tau.shape[0]), dtype=np.complex128)
    g0 = normal_coordinates(seed, 0, tau.shape[0]) if dynamic else None
    for row, c in enumerate(frames):
        if dynamic:
            if c >= 2 ** 31:
                raise ValueError(f"frame index {c} of a dynamic record must be below 2^31")
            a = 2.0 * np.pi * frac(tau * float(c))
            out[row] = g0 * (np.cos(a) - 1j * np.sin(a))
        else:
            out[row] = normal_coordinates(seed, c, tau.shape[0])          # theta = 0: the phase factor is 1
    return out


def displacements_of(positions, basis_index, wavevectors, displacements, C):
    """(n, 3) float64: u_i = sum_m Re[(C[m] E[i, m]) W[m, b_i, :]] of one frame's coefficients C (M,), summed in mode order"""
    r = np.asarray(positions, dtype=np.float64)
    b = np.asarray(basis_index)
    q = np.asarray(wavevectors, dtype=np.float64)
    W = np.asarray(displacements, dtype=np.complex128)
    C = np.asarray(C, dtype=np.complex128)
    u = np.zeros(r.shape, dtype=np.float64)
    for m in range(q.shape[0]):
        x = (q[m, 0] * r[:, 0] + q[m, 1] * r[:, 1]) + q[m, 2] * r[:, 2]
        a = 2.0 * np.pi * frac(x)
        P = C[m] * (np.cos(a) + 1j * np.sin(a))
        Wm = W[m][b]                                        # (n, 3)
        u += P.real[:, None] * Wm.real - P.imag[:, None] * Wm.imag
    return u


def displaced(positions, basis_index, wavevectors, tau, displacements, seed, frame, dynamic=True):
    """positions (n, 3) + the displacements of frame `frame`: one frame, not wrapped, not clipped"""
    r = np.asarray(positions, dtype=np.float64)
    C = mode_coefficients(tau, seed, [frame], dynamic)[0]
    return r + displacements_of(r, basis_index, wavevectors, displacements, C)


def amplitude_scales(frequencies_THz, temperature_K, n_cells, statistics="quantum"):
    """(M,) float64: s_m in Angstrom * sqrt(amu), the rms normal-coordinate amplitude per sqrt(mass):
        quantum:    s^2 = hbar / omega * coth(hbar omega / 2 k_B T) / n_cells
        classical:  s^2 = 2 k_B T / (omega^2 n_cells)
    omega = 2 pi nu.  coth(x) = 1/x + x/3 - ..., so quantum -> classical for k_B T >> h nu."""
    nu = np.asarray(frequencies_THz, dtype=np.float64)
    if statistics not in ("quantum", "classical"):
        raise ValueError(f"statistics must be 'quantum' or 'classical', got {statistics!r}")
    if nu.ndim != 1 or not np.all(np.isfinite(nu)) or np.any(nu < 0):
        raise ValueError("frequencies_THz must be (modes,) finite values >= 0")
    if np.any(nu == 0):
        raise ValueError("frequencies_THz: a mode of frequency 0 has a diverging amplitude (drop the three uniform translations)")
    if isinstance(n_cells, (bool, np.bool_)) or not isinstance(n_cells, (int, np.integer)) or int(n_cells) < 1:
        raise ValueError(f"n_cells must be a positive integer, got {n_cells!r}")
    T = float(temperature_K)
    if not np.isfinite(T) or T < 0 or (T == 0 and statistics == "classical"):
        raise ValueError(f"temperature_K must be finite and >= 0 (> 0 for classical statistics), got {temperature_K!r}")
    omega = 2.0 * np.pi * nu * 1e12                                           # rad / s
    if statistics == "classical":
        s2 = 2.0 * K_B_J_PER_K * T / (omega ** 2 * n_cells)                   # J s^2 = kg m^2
    else:
        coth = 1.0 / np.tanh(HBAR_J_S * omega / (2.0 * K_B_J_PER_K * T)) if T > 0 else np.ones_like(omega)
        s2 = HBAR_J_S / omega * coth / n_cells
    return np.sqrt(s2 / AMU_KG) * 1e10                                        # Angstrom sqrt(amu)


def _positive_int(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


class PhononModes:
    """`n_frames` frames of one structure moved by M phonon modes, as an input of MultisliceCalculator.setup(): what a Trajectory of
    n_frames frames is, without the frames.  `positions` (n_atoms, 3) is the base structure, `basis_index` (n_atoms,) the basis atom
    of every atom, `wavevectors` (M, 3) in cycles / Angstrom, `frequencies` (M,) in cycles per unit of `timestep`, `displacements`
    (M, n_basis, 3) complex in Angstrom per unit normal coordinate, `seed` a non-negative 64-bit integer.  dynamic=True is a
    time-coherent record (one draw of the normal coordinates, every mode advancing by nu * timestep cycles per frame), dynamic=False
    independent snapshots (a new draw per frame).  <u_{i alpha}^2> = 1/2 sum_m |W[m, b_i, alpha]|^2.  configuration(c) is the
    definition of frame c; the device generates the same positions itself, so nothing per frame is stored or copied."""

    def __init__(self, atom_types, positions, box_matrix, basis_index, wavevectors, frequencies, displacements, n_frames, seed=0,
                 timestep=1.0, dynamic=True):
        self.atom_types = np.asarray(atom_types)
        self.positions = np.ascontiguousarray(positions, dtype=np.float64)
        self.box_matrix = np.asarray(box_matrix)
        self.timestep = timestep
        # the messages of Trajectory._validate_shapes where they apply (trajectory.py), as FrozenPhonons
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
        self._n_frames = _positive_int("n_frames", n_frames)
        self.seed = _u64("seed", seed)
        self.dynamic = bool(dynamic)
        if self.dynamic and self._n_frames > 2 ** 31:
            raise ValueError("n_frames of a dynamic record must be at most 2^31")
        ts = float(timestep)
        if not np.isfinite(ts) or ts <= 0:
            raise ValueError(f"timestep must be finite and > 0, got {timestep!r}")

        W = np.asarray(displacements)
        if W.ndim != 3 or W.shape[2] != 3 or W.shape[0] < 1 or W.shape[1] < 1:
            raise ValueError(f"displacements must be (modes >= 1, basis atoms >= 1, 3), got {W.shape}")
        self.displacements = np.ascontiguousarray(W, dtype=np.complex128)
        M, nb = W.shape[:2]
        if not M < 2 ** 31:
            raise ValueError("the number of modes must be below 2^31")
        self.wavevectors = np.ascontiguousarray(wavevectors, dtype=np.float64)
        if self.wavevectors.shape != (M, 3):
            raise ValueError(f"wavevectors must be ({M}, 3), got {self.wavevectors.shape}")
        self.frequencies = np.ascontiguousarray(frequencies, dtype=np.float64)
        if self.frequencies.shape != (M,):
            raise ValueError(f"frequencies must be ({M},), got {self.frequencies.shape}")
        if not np.all(np.isfinite(self.frequencies)) or np.any(self.frequencies < 0):
            raise ValueError("frequencies: every frequency must be finite and >= 0")
        if not np.all(np.isfinite(self.wavevectors)):
            raise ValueError("wavevectors must be finite")
        if not (np.all(np.isfinite(self.displacements.real)) and np.all(np.isfinite(self.displacements.imag))):
            raise ValueError("displacements must be finite")
        b = np.asarray(basis_index)
        if b.shape != (self.n_atoms,):
            raise ValueError(f"basis_index must be ({self.n_atoms},), got {b.shape}")
        if not np.issubdtype(b.dtype, np.integer):
            raise ValueError(f"basis_index must be integers, got {b.dtype}")
        if b.size and (b.min() < 0 or b.max() >= nb):
            raise ValueError(f"basis_index: every index must be in [0, {nb})")
        self.basis_index = np.ascontiguousarray(b, dtype=np.int32)
        self.tau = self.frequencies * ts                    # cycles per frame, rounded once: what the device is given
        if not np.all(np.isfinite(self.tau)):
            raise ValueError("frequencies * timestep must be finite")

    @classmethod
    def from_eigenvectors(cls, atom_types, positions, box_matrix, basis_index, wavevectors, eigenvectors, masses_amu,
                          frequencies_THz, temperature_K, n_cells, n_frames, seed=0, timestep=1.0, dynamic=True,
                          statistics="quantum"):
        """The thermal amplitudes of a harmonic crystal: W[m, b, :] = s_m e[m, b, :] / sqrt(mass_b), with the polarisation vectors
        `eigenvectors` (M, n_basis, 3) normalised over the cell (sum_b |e[m, b]|^2 = 1), `masses_amu` (n_basis,), `n_cells` the
        number of cells in the supercell and s_m of amplitude_scales() (quantum or classical occupation at `temperature_K`).  It
        applies to a mode list that names every (q, branch) of the supercell once: then <u^2> above is the thermal mean-square
        displacement.  `timestep` is in ps, so that frequencies = frequencies_THz.  A mode of frequency 0 raises ValueError: its
        amplitude diverges, the caller drops the three uniform translations."""
        e = np.asarray(eigenvectors, dtype=np.complex128)
        if e.ndim != 3 or e.shape[2] != 3:
            raise ValueError(f"eigenvectors must be (modes, basis atoms, 3), got {e.shape}")
        mass = np.asarray(masses_amu, dtype=np.float64)
        if mass.shape != (e.shape[1],):
            raise ValueError(f"masses_amu must be ({e.shape[1]},), got {mass.shape}")
        if not np.all(np.isfinite(mass)) or np.any(mass <= 0):
            raise ValueError("masses_amu: every mass must be finite and > 0")
        nu = np.asarray(frequencies_THz, dtype=np.float64)
        if nu.shape != (e.shape[0],):
            raise ValueError(f"frequencies_THz must be ({e.shape[0]},), got {nu.shape}")
        s = amplitude_scales(nu, temperature_K, n_cells, statistics)
        W = s[:, None, None] * e / np.sqrt(mass)[None, :, None]
        return cls(atom_types, positions, box_matrix, basis_index, wavevectors, nu, W, n_frames, seed=seed, timestep=timestep,
                   dynamic=dynamic)

    @property
    def n_frames(self) -> int:
        return self._n_frames

    @property
    def n_atoms(self) -> int:
        return len(self.atom_types)

    @property
    def n_modes(self) -> int:
        return self.displacements.shape[0]

    @property
    def n_basis(self) -> int:
        return self.displacements.shape[1]

    @property
    def box_tilts(self) -> np.ndarray:
        return np.array([self.box_matrix[0, 1], self.box_matrix[0, 2], self.box_matrix[1, 2]])

    def mean_square_displacement(self):
        """(n_atoms, 3): <u_{i alpha}^2> = 1/2 sum_m |W[m, b_i, alpha]|^2 in Angstrom^2"""
        return 0.5 * (np.abs(self.displacements) ** 2).sum(axis=0)[self.basis_index]

    def configuration(self, c):
        """(n_atoms, 3) float64: frame c >= 0 (any index: n_frames only says how many a run takes)"""
        return displaced(self.positions, self.basis_index, self.wavevectors, self.tau, self.displacements, self.seed,
                         _u64("frame index", c), self.dynamic)

    def to_trajectory(self, frames=None):
        """The frames (None: 0 .. n_frames - 1) as a Trajectory on the host, 24 B x n_atoms each: for tests and small cases."""
        cs = range(self.n_frames) if frames is None else list(frames)
        pos = np.stack([self.configuration(c) for c in cs]) if len(cs) else np.zeros((0, self.n_atoms, 3))
        return Trajectory(atom_types=self.atom_types, positions=pos, velocities=np.zeros_like(pos), box_matrix=self.box_matrix,
                          timestep=self.timestep)

"""GradientData: what MultisliceCalculator.run_gradient() returns (the definition is adjoint.py)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

import numpy as np


@dataclass
class GradientData:
    """potential  (nx, ny, nz) float64: dL/dV of the total loss, in the layout of Potential.array and of run_gradient(potential=...)
    loss       (P,) float64: the loss of every probe position
    probe      (P, nx, ny) complex64: dL/dpsi_0* per probe with Gradient(probe=True), else None
    sigma      the interaction constant the transmission functions were made with
    xs, ys, zs the axes of `potential`; kind: the loss ("amplitude", "intensity", "poisson"); frame: the frame it was taken at"""
    potential: np.ndarray
    loss: np.ndarray
    sigma: float
    xs: Any = None
    ys: Any = None
    zs: Any = None
    probe: Optional[np.ndarray] = None
    kind: str = "amplitude"
    frame: int = 0
    probe_positions: Any = None
    positions: Optional[np.ndarray] = None      # (n_atoms, 3) float64: dL/dr_a with Gradient(positions=True) (slice-axis column zero), else None
    # the probe recipe backwards; probe_positions above stays the scan positions the run was made at
    probe_position_gradient: Optional[np.ndarray] = None        # (P, 2) float64: dL/d(x_p, y_p) per Angstrom with Gradient(probe_positions=True)
    aberration_gradient: Optional[dict] = None                  # Aberrations field name -> dL/dC_nm per Angstrom, dL/dphi_nm per radian (Gradient(aberrations=True))
    aberration_gradient_cartesian: Optional[np.ndarray] = None  # (14, 2) float64: dL/d(a_j, b_j), summed over the probes

    @property
    def total(self) -> float:
        """the loss summed over the probe positions"""
        return float(np.sum(self.loss))

    def descent_step(self, V, rate):
        """V - rate * dL/dV for an estimate V (nx, ny, nz): one step of plain gradient descent, float64"""
        V = np.asarray(V, dtype=np.float64)
        if V.shape != self.potential.shape:
            raise ValueError(f"descent_step: V {V.shape} does not match the gradient {self.potential.shape}")
        return V - float(rate) * self.potential

    def position_step(self, pos, rate):
        """pos - rate * dL/dr for coordinates pos (n_atoms, 3): one step of plain gradient descent on the atoms, float64 (what the
        next run_gradient(positions=...) takes)"""
        if self.positions is None:
            raise ValueError("position_step: no position gradient (MultisliceCalculator(gradient=Gradient(positions=True)))")
        pos = np.asarray(pos, dtype=np.float64)
        if pos.shape != self.positions.shape:
            raise ValueError(f"position_step: pos {pos.shape} does not match the gradient {self.positions.shape}")
        return pos - float(rate) * self.positions

    def probe_position_step(self, xy, rate):
        """xy - rate * dL/d(x_p, y_p) for scan positions xy (P, 2): one step of plain gradient descent, float64 (what the next
        run_gradient(probe_positions=...) takes)"""
        if self.probe_position_gradient is None:
            raise ValueError("probe_position_step: no scan-position gradient (MultisliceCalculator(gradient=Gradient(probe_positions=True)))")
        xy = np.asarray(xy, dtype=np.float64)
        if xy.shape != self.probe_position_gradient.shape:
            raise ValueError(f"probe_position_step: xy {xy.shape} does not match the gradient {self.probe_position_gradient.shape}")
        return xy - float(rate) * self.probe_position_gradient

    def aberration_step(self, aberrations, rate):
        """a new Aberrations, every field f moved to f - rate * dL/df: one step of plain gradient descent (what the next
        run_gradient(aberrations=...) takes).  rate: a float for every field, or a mapping by field name (a field it does not name
        stays) -- the orders differ by many decades in Angstrom, so one rate rarely serves two of them"""
        from .aberrations import Aberrations
        if self.aberration_gradient is None:
            raise ValueError("aberration_step: no aberration gradient (MultisliceCalculator(gradient=Gradient(aberrations=True)))")
        if not isinstance(aberrations, Aberrations):
            raise ValueError(f"aberration_step: expected an Aberrations object, got {aberrations!r}")
        if isinstance(rate, dict):
            unknown = sorted(set(rate) - set(self.aberration_gradient))
            if unknown:
                raise ValueError(f"aberration_step: unknown fields {unknown} (known: {sorted(self.aberration_gradient)})")
        new = {}
        for name, g in self.aberration_gradient.items():
            r = rate.get(name, 0.0) if isinstance(rate, dict) else rate
            new[name] = getattr(aberrations, name) - float(r) * g
        return Aberrations(**new)

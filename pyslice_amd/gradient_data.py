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

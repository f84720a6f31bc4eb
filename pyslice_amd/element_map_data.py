"""ElementMapData: the result of MultisliceCalculator.run_element_maps() -- the ionisation signal of every channel at every probe
position, slice by slice (ionization.py is the definition)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np

from .stem_data import scan_axes, scan_image


@dataclass
class ElementMapData:
    """per_slice (P, E, nz) float64: the ionisation probability per incident electron of channel e generated in slice s with the probe
    at position p, averaged over the frames; channels the Ionization objects, thickness (nz,) the depth in Angstrom at the exit side
    of each slice; xs / ys the scan grid of image() (default: the distinct probe coordinates)."""
    per_slice: np.ndarray
    channels: List[Any]
    probe_positions: Any
    thickness: np.ndarray
    n_frames: int = 1
    xs: Optional[np.ndarray] = None
    ys: Optional[np.ndarray] = None

    def __post_init__(self):
        self.per_slice = np.asarray(self.per_slice, dtype=np.float64)
        self.thickness = np.asarray(self.thickness, dtype=np.float64)
        if self.per_slice.ndim != 3 or self.per_slice.shape[1] != len(self.channels) or self.per_slice.shape[2] != len(self.thickness):
            raise ValueError(f"per_slice of shape {self.per_slice.shape} for {len(self.channels)} channels and {len(self.thickness)} slices")
        if self.xs is None or self.ys is None:
            self.xs, self.ys = scan_axes(self.probe_positions)

    @property
    def names(self):
        return [c.name for c in self.channels]

    @property
    def signals(self) -> np.ndarray:
        """(P, E): the sum over the slices"""
        return self.cumulative()[..., -1]

    def cumulative(self) -> np.ndarray:
        """(P, E, nz): the signal generated up to and including slice k"""
        return np.cumsum(self.per_slice, axis=-1)

    def index(self, name) -> int:
        """the channel called `name` (the first of that name), or the channel number itself"""
        if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
            if not -len(self.channels) <= int(name) < len(self.channels):
                raise KeyError(f"channel {name} of {len(self.channels)}")
            return int(name) % len(self.channels)
        names = self.names
        if name not in names:
            raise KeyError(f"no channel named {name!r}; channels: {names}")
        return names.index(name)

    def _slice(self, k) -> int:
        nz = self.per_slice.shape[-1]
        if not -nz <= int(k) < nz:
            raise IndexError(f"slice {k} of {nz}")
        return int(k) % nz

    def image(self, name, slice=None) -> np.ndarray:
        """(len(xs), len(ys)) map of channel `name` on the scan grid, every scan point taking its nearest probe's value as
        STEMData.image does; slice=k: the signal up to and including slice k (default: the whole thickness)"""
        e = self.index(name)
        v = self.signals[:, e] if slice is None else self.cumulative()[:, e, self._slice(slice)]
        return scan_image(v, self.probe_positions, self.xs, self.ys)

    def depth_profile(self, name, probe_index) -> np.ndarray:
        """(nz,): what slice s adds to channel `name` with the probe at position probe_index -- the beam-channelling curve, against
        `thickness`"""
        return self.per_slice[int(probe_index), self.index(name)].copy()

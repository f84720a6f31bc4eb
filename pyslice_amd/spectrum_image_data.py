"""Result of MultisliceCalculator.run_spectrum_image(): energy-resolved detector signals over a probe scan.

Everything here is NumPy on the small (P, F, D) result; the sums over the stored pixels were taken on the device
(msl_spectrum_detect).  `image(name, frequency)` is the map TACAWData.spectrum_image(frequency) gives (reference
tacaw_data.py:145-179) restricted to a detector, without the (P, F, nx, ny) intensity ever being held for more than one probe batch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np

from .stem_data import Detector, STEMData, scan_axes, scan_image


@dataclass
class SpectrumImageData:
    """spectra (P, F, D) float64 -- the TACAW intensity inside detector d at frequency bin f and probe p --, frequencies (F,) =
    fftshift(fftfreq(T, dt)) as TACAWData's, the detectors, the run's probe_positions, the scan axes xs / ys, n_frames = T, and
    `stem`: the STEMData of the same propagation when the run asked for it (Spectroscopy(stem=True)), else None."""
    spectra: np.ndarray
    frequencies: np.ndarray
    detectors: List[Detector]
    probe_positions: Any
    n_frames: int
    xs: np.ndarray = None
    ys: np.ndarray = None
    stem: Optional[STEMData] = None

    def __post_init__(self):
        self.spectra = np.asarray(self.spectra, dtype=np.float64)
        self.frequencies = np.asarray(self.frequencies, dtype=np.float64)
        if self.spectra.ndim != 3 or self.spectra.shape[1] != self.frequencies.size or self.spectra.shape[2] != len(self.detectors):
            raise ValueError(f"spectra of shape {self.spectra.shape} for {self.frequencies.size} frequencies and {len(self.detectors)} detectors")
        if self.xs is None or self.ys is None:
            self.xs, self.ys = scan_axes(self.probe_positions)

    def index(self, name: str) -> int:
        for d, det in enumerate(self.detectors):
            if det.name == name:
                return d
        raise KeyError(f"no detector named {name!r} (have {[d.name for d in self.detectors]})")

    def spectrum(self, name: str, probe_index: int = None) -> np.ndarray:
        """(F,): the spectrum of detector `name` at one probe, or its mean over the probes (probe_index=None)"""
        s = self.spectra[:, :, self.index(name)]
        if probe_index is None:
            return s.mean(axis=0)
        if not -s.shape[0] <= probe_index < s.shape[0]:
            raise ValueError(f"Probe index {probe_index} out of range")
        return s[probe_index]

    def per_probe(self, name: str, frequency: float = None, band=None) -> np.ndarray:
        """(P,): detector `name` at the bin nearest `frequency`, or summed over the bins with band[0] <= f <= band[1]"""
        if (frequency is None) == (band is None):
            raise ValueError("give either frequency= or band=(f0, f1)")
        s = self.spectra[:, :, self.index(name)]
        if band is None:
            return s[:, int(np.argmin(np.abs(self.frequencies - frequency)))]
        f0, f1 = float(band[0]), float(band[1])
        sel = (self.frequencies >= f0) & (self.frequencies <= f1)
        if not sel.any():
            raise ValueError(f"no frequency bin inside {(f0, f1)}")
        return s[:, sel].sum(axis=1)

    def image(self, name: str, frequency: float = None, band=None) -> np.ndarray:
        """(len(xs), len(ys)) spectrum image of detector `name`: per_probe() on the scan grid, every scan point taking its nearest
        probe's value (STEMData.image)"""
        return scan_image(self.per_probe(name, frequency, band), self.probe_positions, self.xs, self.ys)

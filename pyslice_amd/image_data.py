"""Frame-averaged images behind an objective lens (MultisliceCalculator(imaging=Imaging(...)).run_images()).

The HIP pass msl_image_add (pyslice_amd/csrc/image.h) applies the lens to the exit spectra of a probe batch, transforms back and adds
|psi|^2 into a float64 accumulator on the device as soon as the slice loop has written them: the (P, T, nx, ny) complex array never
exists, ImageData holds the (P, L, F, nx, ny) frozen-phonon mean only, and everything below is NumPy on that result.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np


@dataclass
class ImageData:
    """Result of MultisliceCalculator.run_images(): intensity (P, L, F, nx, ny) float64 -- the mean over the n_frames MD frames of
    |psi|^2 in the image plane of probe p, layer l, defocus f --, the real-space axes xs / ys (Angstrom), defocus (F,) the values of
    Imaging.defocus_series, layer (L,) slice indices (L = 1: the exit wave), the run's probe_positions and the Imaging request."""
    intensity: np.ndarray
    xs: np.ndarray
    ys: np.ndarray
    defocus: np.ndarray
    layer: np.ndarray
    n_frames: int
    probe_positions: Any
    imaging: Any

    def __post_init__(self):
        self.intensity = np.asarray(self.intensity, dtype=np.float64)
        self.xs, self.ys = np.asarray(self.xs, dtype=np.float64), np.asarray(self.ys, dtype=np.float64)
        self.defocus = np.asarray(self.defocus, dtype=np.float64).reshape(-1)
        self.layer = np.asarray(self.layer).reshape(-1)
        want = (self.intensity.shape[0] if self.intensity.ndim == 5 else -1, len(self.layer), len(self.defocus), len(self.xs), len(self.ys))
        if self.intensity.shape != want:
            raise ValueError(f"intensity has shape {self.intensity.shape}, expected (P, {want[1]}, {want[2]}, {want[3]}, {want[4]})")

    def image(self, defocus_index=0, layer=-1, probe=0) -> np.ndarray:
        """(nx, ny): one image"""
        return self.intensity[probe, layer, defocus_index]

    def diffractogram(self, defocus_index=0, layer=-1, probe=0) -> np.ndarray:
        """(nx, ny): |fftshift(fft2(I - mean(I)))|^2 of one image, on the host"""
        img = self.image(defocus_index, layer, probe)
        return np.abs(np.fft.fftshift(np.fft.fft2(img - img.mean()))) ** 2

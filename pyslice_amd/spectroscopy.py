"""Spectrum imaging: the request object of MultisliceCalculator(spectroscopy=Spectroscopy(...)).run_spectrum_image().

A spectrum image is the TACAW intensity | fftshift_t fft_t(Psi - <Psi>_t) |^2 summed over the stored pixels of a detector, at every
frequency bin and probe position: what vibrational STEM-EELS records through an aperture.  The HIP pass msl_spectrum_detect
(pyslice_amd/csrc/spectrum_detect.h) forms it for every detector at once from the intensity of one probe batch, so a scan needs
neither the (P, T, nx, ny) waves nor their intensity on the device: SpectrumImageData holds the (P, F, D) spectra only.

Spectroscopy(..., segment=L) takes Welch's estimate (welch.py, msl_tacaw_welch) in place of the bare periodogram: L frequency bins
from segments of L frames, which is what tames the variance of the one spectrum a probe position has.
"""
from __future__ import annotations

import numpy as np

from . import welch
from .stem_data import check_detectors


class Spectroscopy:
    """The request: detectors = 1 to 16 stem_data.Detector, every one with signal "intensity" (an amplitude or centre-of-mass
    weight of a TACAW intensity is not defined); stem=True also returns the STEMData run_detectors() gives (the energy-integrated
    signals of the same detectors per frame), from the same propagation.  segment = L (a supported length, welch.supported_lengths()),
    overlap in [0, 1) and window (a name of welch.WINDOWS or L non-negative floats) ask for windowed, segment-averaged spectra with
    L frequency bins: hop = max(1, L - int(overlap L)); with segment=None, overlap and window are ignored."""

    def __init__(self, detectors, stem=False, segment=None, overlap=0.5, window="hann"):
        dets = check_detectors(detectors)
        for d in dets:
            if d.signal != "intensity":
                raise ValueError(f"Spectroscopy: detector {d.name!r} has signal {d.signal!r}; a spectrum image sums the TACAW intensity, "
                                 "only signal='intensity' is defined")
        if not isinstance(stem, (bool, np.bool_)):
            raise ValueError(f"Spectroscopy: stem must be True or False, got {stem!r}")
        self.detectors = dets
        self.stem = bool(stem)
        self.segment = self.hop = self.window = None
        if segment is not None:
            self.segment = welch.check_segment(segment, what="Spectroscopy")
            self.hop = welch.hop_of(self.segment, overlap)
            self.window = welch.window(window, self.segment)

    def __repr__(self):
        names = [d.name for d in self.detectors]
        if self.segment is not None:
            return f"Spectroscopy(detectors={names}, stem={self.stem}, segment={self.segment}, hop={self.hop})"
        return f"Spectroscopy(detectors={names}, stem=True)" if self.stem else f"Spectroscopy(detectors={names})"

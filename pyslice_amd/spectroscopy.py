"""Spectrum imaging: the request object of MultisliceCalculator(spectroscopy=Spectroscopy(...)).run_spectrum_image().

A spectrum image is the TACAW intensity | fftshift_t fft_t(Psi - <Psi>_t) |^2 summed over the stored pixels of a detector, at every
frequency bin and probe position: what vibrational STEM-EELS records through an aperture.  The HIP pass msl_spectrum_detect
(pyslice_amd/csrc/spectrum_detect.h) forms it for every detector at once from the intensity of one probe batch, so a scan needs
neither the (P, T, nx, ny) waves nor their intensity on the device: SpectrumImageData holds the (P, F, D) spectra only.
"""
from __future__ import annotations

import numpy as np

from .stem_data import check_detectors


class Spectroscopy:
    """The request: detectors = 1 to 16 stem_data.Detector, every one with signal "intensity" (an amplitude or centre-of-mass
    weight of a TACAW intensity is not defined); stem=True also returns the STEMData run_detectors() gives (the energy-integrated
    signals of the same detectors per frame), from the same propagation."""

    def __init__(self, detectors, stem=False):
        dets = check_detectors(detectors)
        for d in dets:
            if d.signal != "intensity":
                raise ValueError(f"Spectroscopy: detector {d.name!r} has signal {d.signal!r}; a spectrum image sums the TACAW intensity, "
                                 "only signal='intensity' is defined")
        if not isinstance(stem, (bool, np.bool_)):
            raise ValueError(f"Spectroscopy: stem must be True or False, got {stem!r}")
        self.detectors = dets
        self.stem = bool(stem)

    def __repr__(self):
        names = [d.name for d in self.detectors]
        return f"Spectroscopy(detectors={names}, stem=True)" if self.stem else f"Spectroscopy(detectors={names})"

"""pyslice_amd -- MI355X-native multislice engine behind the PySlice calculator API.

Host code is Python; all arithmetic of the hot path (projected Kirkland potential, probes, the
FFT / transmission / Fresnel slice loop, exit-wave FFT, TACAW time FFT) runs in the C-ABI HIP
library `libmslice.so` (include/mslice.h, pyslice_amd/csrc).  There is no CPU fallback.
"""
from .trajectory import Trajectory
from .thermal import FrozenPhonons, sigma_from_B
from .phonons import PhononModes
from .absorptive import AbsorptivePotential, absorptive_tables, absorptive_transmission, mean_transmission_exact
from .tds import tds_tables, tds_weight, tds_signal
from .wf_data import WFData
from .potentials import Potential, gridFromTrajectory, getZfromElementName, loadKirkland
from .multislice import Probe, Propagate, create_batched_probes, probe_grid, wavelength, m_effective
from .calculators import MultisliceCalculator
from .tacaw_data import TACAWData
from .haadf_data import HAADFData
from .stem_data import Detector, STEMData
from .diffraction_data import Diffraction, DiffractionData
from .polar_data import PolarDetector, PolarData, polar_bins, polar_signals
from .thickness import Thickness
from .aberrations import Aberrations, scherzer_defocus
from .imaging import Imaging
from .image_data import ImageData
from .spectroscopy import Spectroscopy
from .spectrum_image_data import SpectrumImageData
from .tilt import Tilt, Precession
from .bandlimit import BandLimit
from .projection import Projection
from .ionization import Ionization, ionization_weights, ionization_signal
from .element_map_data import ElementMapData
from .dose import Dose, poisson_counts
from .camera import Camera, camera_frames, gaussian_psf, psf_from_mtf
from .coherence import Coherence, blur_scan, chromatic_focal_spread, fwhm_to_sigma
from .adjoint import Gradient, potential_gradient
from .gradient_data import GradientData

__all__ = ["Trajectory", "FrozenPhonons", "sigma_from_B", "PhononModes", "AbsorptivePotential", "absorptive_tables",
           "absorptive_transmission", "mean_transmission_exact", "tds_tables", "tds_weight", "tds_signal", "WFData", "Potential", "gridFromTrajectory", "getZfromElementName", "loadKirkland",
           "Probe", "Propagate", "create_batched_probes", "probe_grid", "wavelength", "m_effective",
           "MultisliceCalculator", "TACAWData", "HAADFData", "Detector", "STEMData", "Diffraction", "DiffractionData",
           "PolarDetector", "PolarData", "polar_bins", "polar_signals", "Thickness",
           "Aberrations", "scherzer_defocus", "Imaging", "ImageData", "Spectroscopy", "SpectrumImageData",
           "Tilt", "Precession", "BandLimit", "Projection", "Ionization", "ionization_weights", "ionization_signal", "ElementMapData",
           "Dose", "poisson_counts", "Camera", "camera_frames", "gaussian_psf", "psf_from_mtf",
           "Coherence", "blur_scan", "chromatic_focal_spread", "fwhm_to_sigma", "Gradient", "potential_gradient", "GradientData"]
__version__ = "0.1.0"

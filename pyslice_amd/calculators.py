"""MultisliceCalculator -- host mirror of src/multislice/calculators.py (the drop-in boundary).

`setup()` and `run()` keep the reference's signatures, defaults and the attributes callers read
(calculators.py:96-161, 163-250).  The per-frame work -- projected potential, probes, slice loop,
exit-wave FFT -- runs in the HIP library; the (P,T,nx,ny) result stays resident on the device
until the end of `run()`, when it is packed into a WFData with the reference's field names,
axis order, fftshift convention and (by default) dtype.

Multi-GPU: when torch.distributed is initialised, MD frames are sharded in contiguous blocks over
the ranks (one process per GPU); there is no collective on the data path, only one gather of the
shards at the end (pyslice_amd/distributed.py).
"""
from __future__ import annotations

import hashlib
import logging
import os
import time
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from . import _native, distributed
from .aberrations import Aberrations
from .bandlimit import as_bandlimit
from .projection import as_projection
from .multislice import Probe, interaction_sigma, wavelength
from .prism import Prism, beams as prism_beams
from .potentials import (TORCH_AVAILABLE, _as_tensor, _device_index, atomic_numbers_of, gridFromTrajectory, loadKirkland, slice_edges,
                         suggest_sampling)
from .thermal import FrozenPhonons
from .thickness import as_thickness
from .tilt import Precession, Tilt
from .phonons import PhononModes
from .absorptive import AbsorptivePotential
from .trajectory import Trajectory
from .wf_data import WFData

if TORCH_AVAILABLE:
    import torch

logger = logging.getLogger(__name__)


def default_frame_batch(n_probes: int, n_slices: int, nx: int, ny: int) -> int:
    """Frames per sequence of launches when the caller does not say (MultisliceCalculator(frame_batch=None), bench.py).

    About 256 images (probes x frames) per launch: a launch of the slice loop is one round of persistent workgroups over the
    256 CUs, and its fixed part (tables into LDS, the first un-prefetched line, the tail of the last round) is amortised over
    the items of a workgroup -- 64 probes x 1024^2 x 200 slices: 277 / 270 / 267 us per 64 images at 1 / 2 / 4 frames per
    launch.  Bounded by 48 GB for the two orientations of the batch's transmission stacks (a sixth of the card; single-probe runs
    still gain from 32 -> 128 frames per launch: 501^2 x 100 slices 160 k -> 167 k slice-steps/s) and 8 GB for the three work
    buffers; setup() halves the batch when the device cannot hold it next to the result."""
    by_images = -(-256 // max(1, n_probes))
    by_stacks = int(48e9 // (16.0 * n_slices * nx * ny))
    by_work = int(8e9 // (24.0 * nx * ny * max(1, n_probes)))
    batch = max(1, min(by_images, by_stacks, by_work))
    if batch >= 16:
        batch -= batch % 16               # whole rounds of work items over the CUs (16-line tiles, 256 CUs x 2 workgroups)
    return batch


def _widen_to_host(view, chunk_bytes=1 << 30):
    """complex64 device tensor (P, T, nx, ny) -> complex128 host tensor, widened on the device in chunks of about 1 GB of
    complex128 (falls back to widening on the host if the device cannot hold one chunk)."""
    # zeros, not empty: the copy engine faults fresh host pages in one by one (84 ms for the 393 MB of a 501 x 491 x 100-frame
    # result), a threaded memset touches them in 6 ms and the copy into touched pages takes 7
    out = torch.zeros(view.shape, dtype=torch.complex128)
    if view.numel() == 0:
        return out
    flat_in = view.reshape(view.shape[0] * view.shape[1], *view.shape[2:]) if view.is_contiguous() else None
    if flat_in is None:                                   # (a frame-sliced view of the engine's buffer: probe by probe)
        rows_in = [view[p] for p in range(view.shape[0])]
        rows_out = [out[p] for p in range(view.shape[0])]
    else:
        rows_in, rows_out = [flat_in], [out.reshape(flat_in.shape)]
    for src, dst in zip(rows_in, rows_out):
        per = max(1, src[0].numel() * 16)
        step = max(1, int(chunk_bytes // per))
        for i in range(0, src.shape[0], step):
            part = src[i:i + step]
            try:
                dst[i:i + step].copy_(part.to(torch.complex128))
            except (RuntimeError, MemoryError):           # no room for the widened chunk on the device
                dst[i:i + step].copy_(part.cpu().to(torch.complex128))
    return out


def _free_device_bytes(dev):
    """free memory of the device in bytes, or None when torch or a device is not there (then the library's allocations decide)"""
    if not (TORCH_AVAILABLE and torch.cuda.is_available()):
        return None
    try:
        return float(torch.cuda.mem_get_info(_device_index(dev))[0])
    except Exception:                                      # pragma: no cover  (no device visible to torch)
        return None


def _positive_pair(name, value, what, cache):
    """k_window / k_bin: None, or two positive integers (not with the frame cache)"""
    if value is None:
        return None
    if len(value) != 2 or int(value[0]) < 1 or int(value[1]) < 1:
        raise ValueError(f"{name} must be two positive pixel counts {what}")
    if cache:
        raise ValueError(f"the frame cache stores full (P,nx,ny,1,1) frames: cache=True cannot be combined with {name}")
    return (int(value[0]), int(value[1]))


class _Progress:
    """the tqdm bar over `total` frames; nothing when it is switched off or tqdm is not installed"""

    def __init__(self, on, total):
        self._bar = None
        if on:
            try:
                from tqdm import tqdm
                self._bar = tqdm(total=total, desc="Processing frames", unit="frame")
            except ImportError:
                pass

    def update(self, n):
        if self._bar is not None:
            self._bar.update(n)

    def close(self):
        if self._bar is not None:
            self._bar.close()


class MultisliceCalculator:

    def __init__(self, device=None, force_cpu=False, *, output="host", dtype="complex128", progress=True,
                 gather="rank0", cache=False, k_window=None, frame_batch=None, k_bin=None, stream_tile=None, layers=None,
                 detectors=None, probe_batch=None, diffraction=None, aberrations=None, imaging=None, prism=None,
                 spectroscopy=None, polar=None, thickness=None, tilt=None, precession=None, tds=False, bandlimit=None,
                 projection=None, ionization=None, coherence=None, gradient=None):
        """
        device / force_cpu: as the reference (calculators.py:41).  There is no CPU path here, so
        force_cpu=True raises.  Keyword-only extras (not in the reference):
          output   "host" (default; WFData.wavefunction_data is a CPU tensor like the reference) or
                   "device" (zero-copy torch view of the library's (P,T,nx,ny) buffer, complex64)
          dtype    "complex128" (default, reference dtype; upcast after download) or "complex64"
          gather   multi-process runs: "rank0" (default), "all" or "none" (keep the local frame shard)
          cache    True: per-frame cache files psi_data/torch_<key>/frame_<i>.npy, (P,nx,ny,1,1) complex128, in the
                   reference's own naming and format (calculators.py:140, 173, 259-260, 311): frames found there are
                   loaded instead of computed (resume), computed frames are written.  Off by default: the reference
                   writes 16*P*nx*ny bytes per frame to the CWD unconditionally (1 GB/frame at C3) and its key ignores
                   the atom positions (stale-hit hazard).
          k_window (wx, wy): keep only the central wx x wy pixels of every exit-wave spectrum (the detector window
                   around k = 0).  wavefunction_data becomes (P,T,wx,wy,1), kxs/kys are cropped to match,
                   and TACAWData / HAADFData work on the window.  Cuts the resident result by nx*ny/(wx*wy) -- the way
                   to hold 2048^2 x 1024-frame runs at all -- and the exit FFT only transforms the columns kept.
          layers   thickness series: 0-based slice indices k whose wave (after the transmission of slice k, before the
                   propagation that follows it: the exit wave of the stack cut after slice k) is recorded as well.  setup()
                   sorts them, drops duplicates and appends nz - 1 (the exit wave, always the last layer); wavefunction_data
                   becomes (P,T,wx,wy,L) and WFData.layer holds the slice indices.  Not with cache, stream_tile or several ranks.
          detectors   STEM mode: a list of up to 16 stem_data.Detector.  run_detectors() then streams the probes through the
                   device in batches and reduces every exit spectrum to its detector values there (msl_detect), so device memory
                   does not grow with the number of probe positions; run() is refused.  Not with cache, layers, stream_tile,
                   k_bin (a bin sums complex pixels: |Psi|^2 of a bin is no detector signal) or several ranks; k_window is
                   allowed (the detectors see the window only).
          diffraction 4D-STEM mode: a diffraction_data.Diffraction(bin=(bx, by)).  run_diffraction() streams the probes through
                   the device as run_detectors() does and reduces every probe batch, there (msl_diffract), to |Psi|^2 summed over
                   the frames of the batch and over every bx x by block of stored pixels: the result is the frame-averaged
                   pattern of every probe position on a pixelated detector, (P, wx/bx, wy/by) float64 on the host.  Same
                   refusals as detectors (k_bin adds complex pixels, the bin here adds intensities); with detectors as well, one
                   propagation feeds both.  setup() raises ValueError when the bin does not divide the stored spectrum.
                   Diffraction(bin, split=True) also returns the elastic part |<Psi>|^2 of every pattern (and the thermal
                   diffuse rest), at the price of one potential build per probe batch and frame (run_diffraction).
                   Diffraction(bin, dose=dose.Dose(...)) returns Poisson counts at that dose, (P, wx/bx, wy/by) uint32, drawn on
                   the device from the frame sums (dose.py is the definition), at the same price.  Not with split=True, thickness,
                   prism, precession, polar, cache, stream_tile or several ranks: NotImplementedError("dose: ... is not built").
          polar    polar-detector mode: a polar_data.PolarDetector(outer, step, inner, n_azimuthal, rotation, per_frame).
                   run_polar() streams the probes through the device as run_detectors() does and reduces every exit spectrum,
                   there (msl_polar_detect), to |Psi|^2 summed over R rings x A sectors: (P, R, A) float64 on the host, the mean
                   over the frames ((P, T, R, A) with per_frame=True), from which any annular, segmented or DPC detector on ring
                   edges is a sum of bins chosen after the run (PolarData.integrate / image / to_stem).  Same refusals as
                   detectors, and not with diffraction, imaging or spectroscopy; with detectors as well, one propagation feeds
                   both (PolarData.stem).  k_window, aberrations, frame_batch, probe_batch and prism are allowed.  setup() raises
                   ValueError when no stored pixel lies in any bin; single empty bins are legal (PolarData.counts).
          probe_batch probes per batch of run_detectors() / run_diffraction() / run_polar() (default: chosen in setup() from free
                   device memory, about 256 images per launch with the frame batch).  Needs detectors, diffraction or polar.
          aberrations an aberrations.Aberrations: every probe of run(), run_streaming_tacaw(), run_detectors() and
                   run_diffraction() is ifft2(mask * ramp * exp(-i chi(k))), built on the device with the probes themselves.
                   Aberrations(defocus=dz) is the reference's Probe.defocus(dz) for dz > 0 (the opposite sign of abTEM's
                   defocus = -C10).  setup(defocus=...) stays stored-only, as in the reference.  No effect on plane waves
                   (aperture == 0).  With cache=True a non-zero set joins the cache key.
          imaging  HRTEM mode: an imaging.Imaging (objective aberrations and aperture, a defocus series, a focal spread).
                   run_images() streams the probes through the device as run_detectors() does and, per probe batch and frame batch,
                   applies the lens to the exit spectra, transforms back and adds |psi|^2 into a float64 accumulator on the device
                   (msl_image_add): the result is the frame-averaged image of every probe and defocus, (P, 1, F, nx, ny) float64 on
                   the host.  A plane-wave run is aperture = 0 in setup().  Imaging(defocus_series=[dz]) is the intensity dz
                   DOWNSTREAM of the exit surface (C10 = +dz, the opposite sign of abTEM's defocus).  run() is refused.  Not with
                   k_window, k_bin, cache, stream_tile, detectors, diffraction, layers (imaging of a thickness series is not built)
                   or several ranks; probe_batch applies.
          prism    a prism.Prism(interpolation): run(), run_detectors() and run_diffraction() build, per frame, the S-matrix of the
                   Bm plane waves inside the aperture (one slice loop per beam instead of one per probe position) and synthesise
                   the exit wave of every probe position from it (msl_smatrix_build / msl_smatrix_probes).  Prism(1) gives the
                   multislice result to fp32 rounding and pays off once there are more probe positions than beams; Prism(f > 1)
                   keeps every f-th beam and a window of 1/f of the cell around each probe -- PRISM's approximation.  The spectra
                   stay on the full grid (zeros outside the window), so k_window, k_bin, aberrations, detectors and probe_batch
                   work as before.  Needs aperture > 0 and an interpolation that divides the grid (setup() raises ValueError).
                   Not built: Diffraction(split=True), imaging, layers, stream_tile, cache, several ranks.
                   Prism(f, crop=True): every probe is synthesised, transformed, stored and reduced on the cropped (nx/fx, ny/fy)
                   grid of a second, potential-less engine (msl_smatrix_probes_cropped).  The results are the uncropped run's
                   spectra at every (fx, fy)-th pixel (prism.crop_index), value for value and NOT rescaled -- a sum over a region is
                   about 1/(fx fy) of the uncropped run's, each cropped pixel standing for fx fy full ones -- on the cropped grid's
                   k axes, with .prism_crop = (fx, fy); k_window, k_bin and Diffraction(bin=) are checked against the cropped grid.
          spectroscopy spectrum-image mode: a spectroscopy.Spectroscopy(detectors=[...]).  run_spectrum_image() streams the probes
                   through the device in batches; per probe batch ALL T frames go into a ring of T frame slots, msl_tacaw turns the
                   ring into the TACAW intensity and msl_spectrum_detect sums it over every detector in one pass: the result is
                   the spectrum of every detector at every probe position, (P, T, D) float64 on the host, and device memory does
                   not grow with the number of probe positions.  The ring and its intensity cost 12 * Pc * T * stored pixels
                   bytes: k_window is the way to make the T frames of a probe fit (the detectors see the window only), setup()
                   halves the probe batch while they do not and raises MemoryError at one probe.  run() and the other run modes
                   are refused.  Allowed with k_window, aberrations, frame_batch, probe_batch; not with detectors, diffraction,
                   imaging, prism, layers, cache, stream_tile, k_bin or several ranks.  Needs at least 2 frames.
          thickness thickness series of the probe-batch modes: a list of 0-based slice indices, or a thickness.Thickness(slices=[...] |
                   every=n, patterns="position" | "pacbed").  Entry k is the wave after the transmission of slice k (the definition
                   of `layers`); setup() sorts the entries, drops duplicates and appends nz - 1, the exit wave.  run_detectors(),
                   run_polar() and run_diffraction() then return, from ONE scan, the signals of every entry on a last axis of
                   length L -- (P, T, D, L), (P, R, A, L), (P, mx, my, L); (mx, my, L) with patterns="pacbed", summed over the
                   probes on the device -- with .layer, .thickness (Angstrom) and .at(i) on the results.  Every tapped layer is
                   reduced on the device at once (msl_set_layer_reduce): one reused block of spectra and a small float64 staging
                   area, whatever L and P.  Needs detectors, polar or diffraction; allowed with k_window, aberrations, probe_batch,
                   frame_batch, FrozenPhonons / PhononModes; not with layers, cache, stream_tile, k_bin, imaging, spectroscopy,
                   prism, Diffraction(split=True) or several ranks.
          tilt     a tilt.Tilt(x_mrad, y_mrad): the beam is inclined to the slice normal (small-angle: the specimen is sheared, free
                   propagation through a slice of thickness dz moves the wave by dz tan(theta), cyclically; the pattern stays
                   centred on the optic axis).  setup() has the device rewrite every propagator table (msl_set_tilt), so every run
                   mode that goes through the slice loop honours it: run(), run_detectors(), run_polar(), run_diffraction() with
                   and without split, run_images(), run_spectrum_image(), layers, thickness, prism, FrozenPhonons / PhononModes.
                   Tilt() is no tilt: the run is bit for bit the one without the argument.  Not built with cache=True (the cache
                   key does not carry the tilt).  |angle| <= 200 mrad.  A tilt along a grid length whose one-pass kernel is a
                   zero-padded convolution or the 2048-point wave kernel runs on the slower two-pass loop (those kernels mirror half
                   of an even table); lengths with a direct kernel next to a multiple of 16 keep the one-pass loop.
          precession a tilt.Precession(angle_mrad, n_azimuth, phase0, centre): run_diffraction(), run_polar() and run_detectors()
                   make one scan per tilt of the cone (one msl_set_tilt between two scans, ordered on the engine's stream) and
                   return the mean of the single-tilt results, accumulated on the host in float64 in tilt order, with the tilts
                   in `.tilts`.  Not with tilt (the cone has a centre).  Not built: the other run modes, stream_tile, cache,
                   several ranks.
          tds      True, with detectors=[...] and an absorptive.AbsorptivePotential(absorption=True) in setup(): run_detectors() also
                   returns what the absorption takes out of the elastic wave and each detector collects -- the thermal diffuse
                   signal, which is most of HAADF -- from the same single pass (tds.py is the definition: the local approximation
                   on top of the second-cumulant model).  STEMData.signals stays the elastic part; .tds_per_slice (P, 1, D, nz),
                   .tds, .total = signals + tds and image(name, part="total" | "elastic" | "tds") carry the rest, with the
                   thickness axis when there is one.  The slice loop then runs on the two-pass loop with a reduction of |psi|^2
                   per slice (msl_set_tds): 3-5 times the time of the elastic scan.  Up to 4 detectors, annuli that read the
                   intensity.  Allowed with tilt, aberrations, k_window, probe_batch, thickness; not built with prism, precession,
                   polar, diffraction, imaging, spectroscopy, layers, cache, stream_tile or several ranks.
          bandlimit a bandlimit.BandLimit(fraction = 2/3), or the fraction itself: anti-aliasing.  setup() has the device mask every
                   propagator table and low-pass every transmission stack after its build (msl_set_bandlimit) to the spatial
                   frequencies below fraction x the Nyquist frequency of the coarser axis; with fraction <= 2/3 no product t psi
                   folds back into the kept band.  Every run mode, source (MD frames, FrozenPhonons, PhononModes,
                   AbsorptivePotential) and tilt, precession, aberrations, k_window, k_bin, probe_batch, frame_batch carry it:
                   it lives in the tables and the stack.  `band_limit_mrad` (after setup()) is the largest angle kept; an
                   aperture beyond it is a ValueError.  The exit spectrum is alias-free inside the band and not zero outside
                   it (bandlimit.propagate_bandlimited).  None: every output is bit for bit that of a run without the argument.
                   Not built with layers, thickness, tds, prism, cache, stream_tile or several ranks.
          projection a projection.Projection(reach = 2.0 A, nodes = 4), or "finite" for that default: the finite projection of DESIGN.md
                   section 4.26.  Every potential build deposits in a slice the part of each atom's 3D Kirkland potential that lies in
                   it -- over R = ceil(reach / slice thickness) slices on either side, z resolved on `nodes` planes per slice
                   (msl_set_projection) -- instead of the whole projected atom in the slice that holds its z.  setup() sets
                   projection_slices (R) and projection_node_spacing (A).  The build costs about 2 (2 R + 1) times the infinite
                   one; the slice loop is unchanged, so every run mode, MD trajectories, FrozenPhonons and PhononModes carry it.
                   None or "infinite": every output is bit for bit that of a run without the argument.  Refused (ValueError): an
                   AbsorptivePotential, tds, cache, stream_tile, several ranks.
          ionization a list of 1 to 8 ionization.Ionization(element, width, cross_section, name): element maps.  run_element_maps()
                   returns, per probe position, channel and slice, the ionisation probability per incident electron in the local
                   approximation -- |psi|^2 inside the specimen against a Gaussian of the channel's width on every atom of its
                   element (ionization.py is the definition) -- as ElementMapData: what an EDX or core-loss EELS map records, and
                   slice by slice the beam-channelling curve.  The scan runs on the two-pass loop with a reduction of |psi|^2 per
                   slice (msl_set_ionization), at a frame batch of 1.  With MD trajectories, FrozenPhonons, PhononModes,
                   AbsorptivePotential, aberrations, tilt, bandlimit and probe_batch.  Not built (NotImplementedError): tds, prism,
                   precession, projection, detectors, polar, diffraction, imaging, spectroscopy, layers, thickness, k_window,
                   k_bin, cache, stream_tile, frame_batch > 1, several ranks.  None: every run is what it is without the argument.
          gradient an adjoint.Gradient(loss, weight, epsilon, probe): run_gradient(data, frame, potential) then returns the derivative
                   of the data-fit loss of the exit patterns with respect to the slice potentials (GradientData; adjoint.py is the
                   definition).  The probes stream in probe_batch; the forward loop keeps the wave arriving at every slice, the
                   residual and the backward loop run on the device (msl_set_adjoint / msl_adjoint_*).  With aberrations, tilt and
                   probe_batch; every other mode: NotImplementedError("gradient: ... is not built").  Gradient(positions=True) adds
                   GradientData.positions, dL/dr_a per atom (msl_adjoint_positions: the potential build backwards), and
                   run_gradient(positions=...) builds from the caller's coordinates.
          coherence a coherence.Coherence(focal_spread, focal_points, source_size, source_points): partial coherence of the probe.
                   Every scan position of run_diffraction() (plain, with Dose, with Dose + Camera), run_detectors() and run_polar()
                   is an ensemble of G = focal_points x source_points^2 member probes, member g at xy + d_g with C10 + delta_g and
                   weight w_g (coherence_members, after setup()), and every result is the weighted sum of the members' INTENSITIES.
                   The members go through the slice loop as ordinary probes of the batch (wave q G + g; msl_set_probe_members);
                   msl_diffract_members / msl_dose_add_members fold the G patterns of a position on the device -- the Poisson draw
                   of a dose run is made from the averaged pattern --, the detector and polar signals are folded on the host in
                   float64, in member order.  The results keep their shapes and carry .coherence.  The cost: G slice loops per
                   position (the potentials are built as often as without); for a source size alone, on a regular raster, without
                   a dose, STEMData.source_blurred(sigma) / coherence.blur_scan is the cheap route.  probe_batch then counts waves:
                   it is rounded down to a multiple of G (ValueError below G), as is the automatic one.  Needs aperture > 0.  With
                   Trajectory, FrozenPhonons, PhononModes, AbsorptivePotential, aberrations, tilt, bandlimit, projection, k_window,
                   probe_batch and frame_batch.  Not built (NotImplementedError): Diffraction(split=True), thickness, layers, prism,
                   precession, tds, ionization, spectroscopy, imaging, run(), run_streaming_tacaw(), cache, stream_tile, several
                   ranks.  Coherence() is off: every run is bit for bit the one without the argument.
        """
        if force_cpu:
            raise NotImplementedError("pyslice_amd has no CPU path (force_cpu=True): use the reference for CPU runs")
        if output not in ("host", "device"):
            raise ValueError("output must be 'host' or 'device'")
        if dtype not in ("complex128", "complex64"):
            raise ValueError("dtype must be 'complex128' or 'complex64'")
        if gather not in ("rank0", "all", "none"):
            raise ValueError("gather must be 'rank0', 'all' or 'none'")
        self._gradient = None
        if gradient is not None:
            from .adjoint import Gradient
            if not isinstance(gradient, Gradient):
                raise ValueError(f"gradient: expected a Gradient object, got {gradient!r}")
            # the adjoint differentiates the plain two-pass loop of one frame, exp(i sigma V) and the full unbinned pattern: every mode
            # that changes the forward model, reduces the patterns or keeps another result has no backward pass
            for what, val in (("dose", getattr(diffraction, "dose", None) is not None), ("bandlimit", bandlimit is not None),
                              ("projection", projection is not None), ("prism", prism is not None), ("coherence", coherence is not None),
                              ("precession", precession is not None), ("k_window", k_window is not None), ("k_bin", k_bin is not None),
                              ("layers", layers is not None), ("thickness", thickness is not None), ("tds", bool(tds)),
                              ("ionization", ionization is not None), ("spectroscopy", spectroscopy is not None),
                              ("imaging", imaging is not None), ("detectors", detectors is not None),
                              ("diffraction", diffraction is not None), ("polar", polar is not None), ("cache", bool(cache)),
                              ("stream_tile", stream_tile is not None),
                              ("frame_batch > 1", frame_batch is not None and int(frame_batch) > 1)):
                if val:
                    raise NotImplementedError(f"gradient: {what} is not built")
            self._gradient = gradient
        self._ionization = None
        if ionization is not None:
            from .ionization import check_ionization
            self._ionization = check_ionization(ionization)
            # a mode of its own on the probe-batch loop: the reductions of the exit spectra, the loops that are not the two-pass
            # loop of one frame, and the stores that keep something else than the per-slice sums are not fed from its pass
            for what, val in (("tds", bool(tds)), ("prism", prism is not None), ("precession", precession is not None),
                              ("projection", projection is not None), ("detectors", detectors is not None), ("polar", polar is not None),
                              ("diffraction", diffraction is not None), ("imaging", imaging is not None),
                              ("spectroscopy", spectroscopy is not None), ("layers", layers is not None),
                              ("thickness", thickness is not None), ("k_window", k_window is not None), ("k_bin", k_bin is not None),
                              ("cache", bool(cache)), ("stream_tile", stream_tile is not None),
                              ("frame_batch > 1", frame_batch is not None and int(frame_batch) > 1)):
                if val:
                    raise NotImplementedError(f"ionization: {what} is not built")
        self._coherence = None                  # a Coherence with more than one member; None: the coherent probe of today
        self.coherence_members = None           # (offsets (G, 2), defocus (G,), weights (G,)) of the members; None when off
        if coherence is not None:
            from .coherence import Coherence
            if not isinstance(coherence, Coherence):
                raise ValueError(f"coherence: expected a Coherence object, got {coherence!r}")
            if not coherence.is_off:
                # the members are waves of the probe batch, folded by the reductions of the exit patterns: the modes that reduce
                # elsewhere, hold every wave, synthesise their probes or average over several scans are not fed from that fold
                for what, val in (("Diffraction(split=True)", getattr(diffraction, "split", False)), ("thickness", thickness is not None),
                                  ("layers", layers is not None), ("prism", prism is not None), ("precession", precession is not None),
                                  ("tds", bool(tds)), ("ionization", ionization is not None), ("spectroscopy", spectroscopy is not None),
                                  ("imaging", imaging is not None), ("cache", bool(cache)), ("stream_tile", stream_tile is not None),
                                  ("run() / run_streaming_tacaw() (give detectors=[...], polar=PolarDetector(...) or "
                                   "diffraction=Diffraction(...))", detectors is None and diffraction is None and polar is None)):
                    if val:
                        raise NotImplementedError(f"coherence: {what} is not built")
                self._coherence = coherence
                self.coherence_members = coherence.members()
        self._dose = getattr(diffraction, "dose", None)
        self._camera = getattr(diffraction, "camera", None)     # (only with a dose: Diffraction refuses it otherwise, so it inherits the refusals below)
        self.electrons_per_probe = None         # setup(): the electrons per probe position of a dose run
        if self._dose is not None:
            # counts are drawn from the per-probe frame sums of the exit patterns on the device: the modes that reduce elsewhere, keep
            # their own result loop or average over several scans are not fed from that accumulator
            for what, val in (("thickness", thickness is not None), ("prism", prism is not None), ("precession", precession is not None),
                              ("polar", polar is not None), ("cache", bool(cache)), ("stream_tile", stream_tile is not None)):
                if val:
                    raise NotImplementedError(f"dose: {what} is not built")
        self.device = device
        self._output, self._dtype, self._progress, self._gather = output, dtype, progress, gather
        self._cache = bool(cache)
        self._k_window = k_window = _positive_pair("k_window", k_window, "(wx, wy)", cache)
        self._k_bin = k_bin = _positive_pair("k_bin", k_bin, "(bx, by)", cache)
        if stream_tile is not None and int(stream_tile) < 1:
            raise ValueError("stream_tile must be a positive frame count")
        if stream_tile is not None and cache:
            raise ValueError("stream_tile cannot be combined with cache=True")
        self._stream_tile = None if stream_tile is None else int(stream_tile)
        if frame_batch is not None and int(frame_batch) < 1:
            raise ValueError("frame_batch must be a positive frame count")
        self._frame_batch = None if frame_batch is None else int(frame_batch)
        if layers is not None:
            if cache:
                raise ValueError("the frame cache has no layer axis: cache=True cannot be combined with layers")
            if stream_tile is not None:
                raise ValueError("streaming TACAW keeps the exit wave only: stream_tile cannot be combined with layers")
            layers = list(layers)
        self._layers_arg = layers
        if thickness is not None:
            thickness = as_thickness(thickness)
            if detectors is None and polar is None and diffraction is None:
                raise ValueError("thickness applies to run_detectors(), run_polar() and run_diffraction(): give detectors=[...], "
                                 "polar=PolarDetector(...) or diffraction=Diffraction(...) (layers=[...] keeps the spectra of run())")
            for what, val in (("layers", layers is not None), ("cache", cache), ("stream_tile", stream_tile is not None),
                              ("k_bin", k_bin is not None)):
                if val:
                    raise ValueError(f"thickness cannot be combined with {what}")
            for what, val in (("imaging", imaging is not None), ("spectroscopy", spectroscopy is not None), ("prism", prism is not None),
                              ("Diffraction(split=True)", getattr(diffraction, "split", False))):
                if val:
                    raise NotImplementedError(f"thickness with {what} is not built")
        self._thickness_arg = thickness
        self._thickness = None                  # validated slice indices (setup), nz - 1 last; None without a thickness series
        if polar is not None:
            from .polar_data import PolarDetector
            if not isinstance(polar, PolarDetector):
                raise ValueError(f"polar: expected a PolarDetector object, got {polar!r}")
            # a probe-batch mode like detectors; the modes with a result loop of their own are not fed from its pass
            for what, val in (("cache", cache), ("layers", layers is not None), ("stream_tile", stream_tile is not None),
                              ("k_bin", k_bin is not None), ("diffraction", diffraction is not None), ("imaging", imaging is not None),
                              ("spectroscopy", spectroscopy is not None)):
                if val:
                    raise ValueError(f"polar cannot be combined with {what}"
                                     + (" (a bin sums complex pixels: |Psi|^2 of a bin is no detector signal)" if what == "k_bin" else ""))
        self._polar = polar
        if spectroscopy is not None:
            from .spectroscopy import Spectroscopy
            if not isinstance(spectroscopy, Spectroscopy):
                raise ValueError(f"spectroscopy: expected a Spectroscopy object, got {spectroscopy!r}")
            # a spectrum image owns the detectors and the result ring (T slots of one probe batch), and needs the exit wave of
            # every frame of a probe at once
            for what, val in (("detectors", detectors is not None), ("diffraction", diffraction is not None),
                              ("imaging", imaging is not None), ("prism", prism is not None), ("layers", layers is not None),
                              ("cache", cache), ("stream_tile", stream_tile is not None), ("k_bin", k_bin is not None)):
                if val:
                    raise ValueError(f"spectroscopy cannot be combined with {what}")
        self._spectroscopy = spectroscopy
        if prism is not None:
            if not isinstance(prism, Prism):
                raise ValueError(f"prism: expected a Prism object, got {prism!r}")
            for what, val in (("cache", cache), ("layers", layers is not None), ("stream_tile", stream_tile is not None),
                              ("imaging", imaging is not None)):
                if val:
                    raise NotImplementedError(f"prism with {what} is not built")
            if diffraction is not None and getattr(diffraction, "split", False):
                raise NotImplementedError("prism with Diffraction(split=True) is not built: the elastic / thermal-diffuse split of "
                                          "PRISM waves")
        self._prism = prism
        if (probe_batch is not None and detectors is None and diffraction is None and imaging is None and spectroscopy is None
                and polar is None and ionization is None and gradient is None):
            raise ValueError("probe_batch applies to detector and diffraction runs only: give detectors=[...] or diffraction=Diffraction(...)")
        if probe_batch is not None and int(probe_batch) < 1:
            raise ValueError("probe_batch must be a positive probe count")
        if diffraction is not None:
            from .diffraction_data import Diffraction
            if not isinstance(diffraction, Diffraction):
                raise ValueError(f"diffraction: expected a Diffraction object, got {diffraction!r}")
        # the probe-batch modes keep one probe batch x one frame batch of full complex spectra on the device, and nothing else
        for mode, given, why_not_k_bin in (
                ("detectors", detectors, " (a bin sums complex pixels: |Psi|^2 of a bin is no detector signal)"),
                ("diffraction", diffraction, " (a bin sums complex pixels; Diffraction(bin=...) sums their intensities)")):
            for what, val in (("cache", cache), ("layers", layers is not None), ("stream_tile", stream_tile is not None),
                              ("k_bin", k_bin is not None)):
                if given is not None and val:
                    raise ValueError(f"{mode} cannot be combined with {what}" + (why_not_k_bin if what == "k_bin" else ""))
        if detectors is not None:
            from .stem_data import check_detectors
            detectors = check_detectors(detectors)
        self._detectors, self._diffraction = detectors, diffraction
        if imaging is not None:
            from .imaging import Imaging
            if not isinstance(imaging, Imaging):
                raise ValueError(f"imaging: expected an Imaging object, got {imaging!r}")
            # an image needs every pixel of the exit spectrum, and its own loop over the probe batches
            for what, val in (("k_window", k_window is not None), ("k_bin", k_bin is not None), ("cache", cache),
                              ("stream_tile", stream_tile is not None), ("detectors", detectors is not None),
                              ("diffraction", diffraction is not None)):
                if val:
                    raise ValueError(f"imaging cannot be combined with {what}")
            if layers is not None:
                raise ValueError("imaging of thickness-series layers is not built")
        self._imaging = imaging
        if aberrations is not None and not isinstance(aberrations, Aberrations):
            raise ValueError(f"aberrations: expected an Aberrations object, got {aberrations!r}")
        self._aberrations = aberrations
        self._probe_batch = None if probe_batch is None else int(probe_batch)
        if tilt is not None and not isinstance(tilt, Tilt):
            raise ValueError(f"tilt: expected a Tilt object, got {tilt!r}")
        if precession is not None:
            if not isinstance(precession, Precession):
                raise ValueError(f"precession: expected a Precession object, got {precession!r}")
            if tilt is not None:
                raise ValueError("precession cannot be combined with tilt: the cone has a centre, Precession(..., centre=Tilt(...))")
            for what, val in (("stream_tile", stream_tile is not None), ("cache=True", cache)):
                if val:
                    raise NotImplementedError(f"precession with {what} is not built")
            if (detectors is None and diffraction is None and polar is None) or imaging is not None or spectroscopy is not None \
                    or layers is not None:
                raise NotImplementedError("precession with run(), layers, run_images(), run_spectrum_image() or run_streaming_tacaw() is not "
                                          "built: give detectors=[...], polar=PolarDetector(...) or diffraction=Diffraction(...)")
        if cache and tilt is not None and not tilt.is_zero:
            raise NotImplementedError("cache=True with a tilt is not built: the cache key does not carry the tilt")
        self._tilt, self._precession = tilt, precession
        self._tds = bool(tds)
        if self._tds:
            from .tds import check_tds_detectors
            check_tds_detectors(detectors)
            for what, val in (("prism", prism is not None), ("precession", precession is not None), ("polar", polar is not None),
                              ("diffraction", diffraction is not None), ("imaging", imaging is not None),
                              ("spectroscopy", spectroscopy is not None), ("layers", layers is not None), ("cache", cache),
                              ("stream_tile", stream_tile is not None)):
                if val:
                    raise NotImplementedError(f"tds: {what} is not built")
        self._bandlimit = bandlimit = as_bandlimit(bandlimit)
        if bandlimit is not None:
            # layers / thickness: the tap inverts the propagator with conj(P), which a masked table does not have; tds: its weights
            # come from the unlimited Omega; prism: the beams and the window do not state the limit; cache: the key does not carry it
            for what, val in (("layers", layers is not None), ("thickness", thickness is not None), ("tds", self._tds),
                              ("prism", prism is not None), ("cache=True", cache), ("stream_tile", stream_tile is not None)):
                if val:
                    raise NotImplementedError(f"bandlimit: {what} is not built")
        self.band_limit_mrad = None             # setup(): the largest scattering angle the band limit keeps
        self._projection = as_projection(projection)
        if self._projection is not None:
            # tds: its tables are those of the absorptive potential; cache: the key does not carry the projection; stream_tile: the
            # streaming run shards frames over ranks with engines of its own set-up
            for what, val in (("tds", self._tds), ("cache", cache), ("stream_tile", stream_tile is not None)):
                if val:
                    raise ValueError(f"projection cannot be combined with {what}")
        self.projection_slices = None           # setup(): R, the reach in slices
        self.projection_node_spacing = None     # setup(): dz / nodes in Angstrom
        self._precessing = False                # inside the tilt loop of a precession run
        self._layers = None                     # validated slice indices (setup), nz - 1 last
        self._engine = None
        self._beam_engine = None                # Prism(f, crop=True): the full-grid engine of the S-matrix; _engine is the cropped one
        self._crop = None                       # (fx, fy) of a cropped PRISM run (setup)
        # reference calculators.py:70-76 (display names for Z <= 36)
        self.element_map = {
            1: 'H', 2: 'He', 3: 'Li', 4: 'Be', 5: 'B', 6: 'C', 7: 'N', 8: 'O', 9: 'F', 10: 'Ne', 11: 'Na', 12: 'Mg',
            13: 'Al', 14: 'Si', 15: 'P', 16: 'S', 17: 'Cl', 18: 'Ar', 19: 'K', 20: 'Ca', 21: 'Sc', 22: 'Ti', 23: 'V',
            24: 'Cr', 25: 'Mn', 26: 'Fe', 27: 'Co', 28: 'Ni', 29: 'Cu', 30: 'Zn', 31: 'Ga', 32: 'Ge', 33: 'As',
            34: 'Se', 35: 'Br', 36: 'Kr'}

    def _generate_cache_key(self, trajectory, aperture, voltage_eV, slice_thickness, sampling, probe_positions):
        """reference calculators.py:78-94 (same recipe, so reference and build name the same directory)."""
        params = {
            'n_frames': trajectory.n_frames, 'n_atoms': trajectory.n_atoms,
            'box_matrix': trajectory.box_matrix.tolist(), 'atom_types': trajectory.atom_types.tolist(),
            'aperture': aperture, 'voltage_eV': voltage_eV, 'slice_thickness': slice_thickness,
            'sampling': sampling, 'probe_positions': probe_positions, 'backend': 'pytorch'}
        ab = getattr(self, "_aberrations", None)
        if ab is not None and not ab.is_zero:           # (without aberrations the key stays the one the reference computes)
            params['aberrations'] = tuple(map(tuple, ab.as_polar().tolist()))
        return hashlib.md5(str(sorted(params.items())).encode()).hexdigest()[:12]

    def setup(
        self,
        trajectory: Trajectory,
        aperture: float = 0.0,
        voltage_eV: float = 60e3,
        defocus: float = 0.0,
        slice_thickness: float = 0.5,
        sampling: float = 0.1,
        probe_positions: Optional[List[Tuple[float, float]]] = None,
        batch_size: int = 10,
        save_path: Optional[Path] = None,
        cleanup_temp_files: bool = False,
        slice_axis: int = 2,
    ):
        """reference calculators.py:96-161 -- same arguments, same defaults, same attributes.

        (not in the reference) `trajectory` may be a thermal.FrozenPhonons: its n_configs Einstein-model configurations take the
        place of the MD frames in every run mode, generated on the device from the resident base structure (msl_set_structure
        once, msl_build_thermal per frame batch) instead of being copied from a (T, n_atoms, 3) host array.  Not built with it:
        cache=True, stream_tile / run_streaming_tacaw(), several ranks (NotImplementedError).

        It may also be a phonons.PhononModes: its n_frames frames, synthesised on the device from a set of phonon modes
        (msl_set_structure and msl_set_modes once, msl_build_modes per frame batch) -- a time-coherent record whose TACAW spectrum
        shows the dispersion, or independent correlated snapshots.  The same run modes, the same three refusals.

        Or an absorptive.AbsorptivePotential: ONE frame whose transmission functions are the thermal average exp(i sigma Vbar -
        sigma^2 Omega) (msl_set_absorption once; the build is the ordinary one of the host positions).  Every run mode but
        spectroscopy; the same three refusals."""
        # a generated source: frames made on the device by index from a resident structure, never read from a host array
        self._generated = trajectory if isinstance(trajectory, (FrozenPhonons, PhononModes)) else None
        if self._generated is not None:
            kind = "phonon modes" if isinstance(trajectory, PhononModes) else "frozen phonons"
            for what, val in (("cache=True", self._cache), ("stream_tile / run_streaming_tacaw()", self._stream_tile is not None),
                              ("a run over several ranks", distributed.rank_world()[1] > 1)):
                if val:
                    raise NotImplementedError(f"{kind}: {what} is not built")
        # (not in the reference) an absorptive.AbsorptivePotential: one frame whose builds go through msl_set_absorption
        self._absorptive = trajectory if isinstance(trajectory, AbsorptivePotential) else None
        if self._absorptive is not None:
            for what, val in (("cache=True", self._cache), ("stream_tile / run_streaming_tacaw()", self._stream_tile is not None),
                              ("a run over several ranks", distributed.rank_world()[1] > 1),
                              ("spectroscopy (one frame has no spectrum)", self._spectroscopy is not None)):
                if val:
                    raise NotImplementedError(f"absorptive potential: {what} is not built")
        if getattr(self, "_projection", None) is not None:
            if self._absorptive is not None:
                raise ValueError("projection cannot be combined with an AbsorptivePotential: its Debye-Waller and absorptive tables are "
                                 "infinite projections")
            if distributed.rank_world()[1] > 1:
                raise ValueError("projection cannot be combined with a run over several ranks")
        if getattr(self, "_tds", False):
            if self._absorptive is None or not self._absorptive.absorption:
                raise ValueError("tds=True needs an absorptive.AbsorptivePotential(absorption=True) in setup(): the TDS signal is what "
                                 "its absorption takes out of the elastic wave")
            if distributed.rank_world()[1] > 1:
                raise NotImplementedError("tds: a run over several ranks is not built")
        if getattr(self, "_ionization", None) is not None and distributed.rank_world()[1] > 1:
            raise NotImplementedError("ionization: a run over several ranks is not built")
        if getattr(self, "_gradient", None) is not None:
            for what, val in (("FrozenPhonons", isinstance(trajectory, FrozenPhonons)), ("PhononModes", isinstance(trajectory, PhononModes)),
                              ("AbsorptivePotential", isinstance(trajectory, AbsorptivePotential)),
                              ("a run over several ranks", distributed.rank_world()[1] > 1)):
                if val:
                    raise NotImplementedError(f"gradient: {what} is not built")
        if getattr(self, "_coherence", None) is not None:
            if distributed.rank_world()[1] > 1:
                raise NotImplementedError("coherence: a run over several ranks is not built")
            if not aperture > 0:
                raise ValueError("coherence needs a convergent probe: setup(aperture > 0) (a plane wave has neither a defocus nor a "
                                 "position)")
        self.trajectory = trajectory
        self.aperture = aperture
        self.voltage_eV = voltage_eV
        self.defocus = defocus                  # stored, never applied -- as in the reference (:129)
        self.slice_thickness = slice_thickness
        self.sampling = sampling
        self.probe_positions = probe_positions
        self.save_path = save_path
        self.cleanup_temp_files = cleanup_temp_files
        self.slice_axis = slice_axis

        cache_key = self._generate_cache_key(trajectory, aperture, voltage_eV, slice_thickness, sampling, probe_positions)
        self.output_dir = Path("psi_data") / f"torch_{cache_key}"    # created only when the frame cache is switched on
        if self._cache:
            self.output_dir.mkdir(parents=True, exist_ok=True)

        xs, ys, zs, lx, ly, lz = gridFromTrajectory(trajectory, sampling=sampling, slice_thickness=slice_thickness)
        nx, ny, nz = len(xs), len(ys), len(zs)
        self.xs, self.ys, self.zs = xs, ys, zs
        self.lx, self.ly, self.lz = lx, ly, lz
        self.nx, self.ny, self.nz = nx, ny, nz
        self.dx = xs[1] - xs[0]
        self.dy = ys[1] - ys[0]
        self._bl_cuts = None
        if self._bandlimit is not None:
            if distributed.rank_world()[1] > 1:
                raise NotImplementedError("bandlimit: a run over several ranks is not built")
            self._bl_cuts = self._bandlimit.cuts(nx, ny, self.dx, self.dy)
            self.band_limit_mrad = self._bandlimit.max_angle_mrad(wavelength(voltage_eV), nx, ny, self.dx, self.dy)
            if aperture > self.band_limit_mrad:
                raise ValueError(f"bandlimit: the aperture of {aperture:g} mrad lies beyond the band limit of {self.band_limit_mrad:.4g} mrad "
                                 "(band_limit_mrad): the probe would lose its outer zone at the first propagation")
        self._layers = self._check_layers(len([xs, ys, zs][slice_axis]), distributed.rank_world()[1])
        self._prism_Bm = 0
        self._crop = None
        if self._prism is not None:
            self._check_prism(nx, ny, distributed.rank_world()[1])
        # (not in the reference) a line length without a slice-loop kernel of its own costs 2-4 x: name a nearby sampling that has one
        hint = suggest_sampling(trajectory, sampling)
        self.grid_hint = None if hint is None else (
            f"grid {nx} x {ny}: at least one axis runs as a zero-padded convolution; sampling={hint[0]:.6g} gives {hint[1]} x {hint[2]} "
            f"on direct kernels (modelled faster although finer)")
        if self.grid_hint and self._progress and distributed.rank_world()[0] == 0:
            print(self.grid_hint)

        if self.probe_positions is None:
            self.probe_positions = [(lx / 2, ly / 2)]
        self._rank, self._world = distributed.rank_world()
        if self._precession is not None and self._world > 1:
            raise NotImplementedError("precession: a run over several ranks is not built")
        if self._spectroscopy is not None:
            self._setup_spectrum_image(trajectory, slice_axis)
            return
        if (self._detectors is not None or self._diffraction is not None or self._imaging is not None or self._polar is not None
                or self._ionization is not None or getattr(self, "_gradient", None) is not None):
            self._setup_probe_batches(trajectory, slice_axis)
            return
        n_slices = self._setup_run(trajectory, slice_axis)
        # frame shard of this rank (contiguous block) and the device that serves it
        self._frames = distributed.shard_frames(self.n_frames, self._world, self._rank)
        dev = self.device
        if dev is None and self._world > 1:
            dev = int(os.environ.get("LOCAL_RANK", self._rank))
        batch = self._frame_batch
        if batch is None:
            batch = default_frame_batch(self.n_probes, n_slices, nx, ny)
        batch = 1 if (self._cache or self._prism is not None) else max(1, min(batch, len(self._frames)))
        slots = max(1, len(self._frames))
        if self._stream_tile is not None:
            slots = max(1, min(self._stream_tile, slots))
            batch = min(batch, slots)
        if self._k_bin is not None:
            wx, wy = self._stored_window()
            if wx % self._k_bin[0] or wy % self._k_bin[1]:
                raise ValueError(f"the stored spectrum {wx} x {wy} is not a multiple of k_bin {self._k_bin}")
        if self._frame_batch is None and batch > 1:            # (an explicit frame_batch is honoured as is)
            free_b = _free_device_bytes(dev)
            if free_b is not None:
                batch = self._fit_frame_batch(free_b, batch, slots)
        self._check_layer_memory(dev, slots)

        # The frame batch costs batch x (two orientations of the transmission stack + three work buffers): when the device cannot
        # hold it next to the (P, T_local, wx, wy) result -- a result near capacity, a shared or smaller GPU -- halve it down to one
        # frame per launch sequence instead of failing a run that fits without batching (an explicit frame_batch is honoured as is)
        def shrink(n_probes, slots, batch):
            if self._frame_batch is not None or batch <= 1:
                return None
            batch = max(1, batch // 2)
            if self._stream_tile is not None:
                batch = min(batch, slots)
            logger.info(f"device memory: frame batch reduced to {batch}")
            return n_probes, slots, batch
        self._create_engine(self.n_probes, slots, batch, shrink, device=_device_index(dev), k_bin=self._k_bin)
        if len(self._layers) > 1:
            self._engine.set_layers(self._layers[:-1])
        self._configure_engine()
        if self._prism is not None:                             # (the probes are synthesised from the S-matrix: none to set)
            self._source_engine().smatrix_begin(self._prism.interpolation, self.aperture)
            return
        self._engine.set_probes(self.aperture, np.asarray(self.probe_positions, dtype=np.float64))

    def _setup_probe_batches(self, trajectory, slice_axis):
        """setup() of a run that streams probe batches (detectors, diffraction, polar): every check on the host first, then an
        engine of Pc <= P probes x one frame batch of result slots, then the detector memberships and the polar bin map onto it"""
        if self._world > 1 and self._thickness_arg is not None:
            raise NotImplementedError("thickness: runs over several ranks are not built")
        if self._world > 1 and self._dose is not None:
            raise NotImplementedError("dose: several ranks is not built")
        if self._dose is not None:                              # (per_area: ValueError for a scan that is no regular raster)
            self.electrons_per_probe = float(self._dose.electrons(self.probe_positions))
            if len(self.probe_positions) > 2 ** 32:
                raise ValueError("dose: the probe index is a 32-bit word of the counter")
        if self._world > 1:
            mode = "detectors" if self._detectors is not None else ("diffraction" if self._diffraction is not None else
                                                                    ("polar" if self._polar is not None else "imaging"))
            raise NotImplementedError(f"{mode}: runs over several ranks are not supported (run_detectors() / run_diffraction() / "
                                      "run_polar() are single-process)")
        if self._diffraction is not None:
            wx, wy = self._stored_window()
            bx, by = self._diffraction.bin
            if wx % bx or wy % by:
                raise ValueError(f"the stored spectrum {wx} x {wy} is not a multiple of the diffraction bin {bx} x {by}")
        if self._detectors is not None:
            from .stem_data import detector_bitmask
            kxs, kys = self._k_axes()
            bits = detector_bitmask(self._detectors, kxs, kys, wavelength(self.voltage_eV))
            for d, det in enumerate(self._detectors):
                if not ((bits >> d) & 1).any():
                    raise ValueError(f"detector {det.name!r} contains no stored pixel of the {len(kxs)} x {len(kys)} spectrum")
            self._det_bits = bits
        if self._polar is not None:
            from .polar_data import bin_counts, polar_bins
            pkx, pky = self._k_axes()
            self._polar_bins = polar_bins(self._polar, pkx, pky, wavelength(self.voltage_eV))
            self._polar_counts = bin_counts(self._polar_bins, self._polar.n_bins)
            if not self._polar_counts.any():
                raise ValueError(f"polar: no stored pixel of the {len(pkx)} x {len(pky)} spectrum lies between {self._polar.inner:g} and "
                                 f"{self._polar.edges[-1]:g} mrad")
        grad = getattr(self, "_gradient", None)
        if grad is not None and grad.weight is not None and grad.weight.shape != (self.nx, self.ny):
            raise ValueError(f"gradient: weight {grad.weight.shape} does not match the {self.nx} x {self.ny} pattern")
        n_slices = self._setup_run(trajectory, slice_axis)
        self._frames = list(range(self.n_frames))
        self._thickness = None if self._thickness_arg is None else self._thickness_arg.resolve(n_slices)
        # Pc x frame batch near the ~256 images per launch of default_frame_batch: 256 probes x 1 frame for a scan, all probes x
        # ceil(256 / P) frames for a few (an explicit probe_batch is honoured as is)
        auto = self._probe_batch is None
        # with a Coherence the engine's probes are WAVES, G members per position: whole positions per batch
        G = self._members_G()
        if not auto and self._probe_batch < G:
            raise ValueError(f"coherence: probe_batch={self._probe_batch} is below the G = {G} member probes of one position")
        Pc = min(self.n_probes * G, 256 if auto else self._probe_batch) // G * G
        batch = self._frame_batch if self._frame_batch is not None else default_frame_batch(Pc, n_slices, self.nx, self.ny)
        # (the S-matrix holds one frame; so does the weight stack of the ionisation channels)
        batch = 1 if (self._prism is not None or self._ionization is not None or grad is not None) else max(1, min(batch, self.n_frames))
        free_b = _free_device_bytes(self.device) if auto else None
        if free_b is not None:
            Pc = max(G, self._fit_probe_batch(free_b, Pc, batch) // G * G)

        def shrink(Pc, slots, batch):                           # the probe batch first, then the frame batch and with it the ring
            if not auto or (Pc <= G and batch <= 1):
                return None
            if Pc > G:
                Pc = max(G, Pc // 2 // G * G)
            else:
                batch = max(1, batch // 2)
            logger.info(f"device memory: probe batch {Pc}, frame batch {batch}")
            return Pc, batch, batch

        def furnish():
            """what the engine of a probe-batch run allocates after msl_create, inside the shrink-and-retry of _create_engine: a
            thickness series whose block, tap buffer and staging do not fit is tried again at the next smaller probe batch"""
            self._configure_engine()                            # (the aberrations are read by the set_probes of every probe batch)
            if self._detectors is not None:
                self._engine.set_detectors(bits.reshape(-1), [d.signal for d in self._detectors], kxs, kys)
            if self._tds:                                       # (before the first build: its tables are those of the detectors)
                from .tds import tds_members
                self._engine.set_tds(tds_members(self._detectors, self.nx, self.ny, self.dx, self.dy, wavelength(self.voltage_eV)),
                                     len(self._detectors))
            if self._ionization is not None:                    # (before the first build, which then makes the weight stack)
                self._engine.set_ionization(self._ionization)
            if self._polar is not None:
                self._engine.set_polar(self._polar_bins.reshape(-1), self._polar.n_bins)
            if grad is not None:                                # (the wave stack of the probe batch: what a smaller batch makes fit)
                self._engine.set_adjoint(grad.kind, grad.epsilon, grad.weight)
            if self._thickness is not None and len(self._thickness) > 1:    # (the exit wave alone needs no tap: the plain reductions)
                pacbed = self._diffraction is not None and self._thickness_arg.patterns == "pacbed"
                what = ((_native.LR_DETECT if self._detectors is not None else 0) | (_native.LR_POLAR if self._polar is not None else 0)
                        | (0 if self._diffraction is None else (_native.LR_PACBED if pacbed else _native.LR_DIFFRACT)))
                self._engine.set_layer_reduce(self._thickness[:-1], what,
                                              bin=(1, 1) if self._diffraction is None else self._diffraction.bin)
            if self._prism is not None:
                self._source_engine().smatrix_begin(self._prism.interpolation, self.aperture)
        self._create_engine(Pc, batch, batch, shrink, furnish=furnish, device=_device_index(self.device))
        self.probe_batch = self._engine.n_probes

    def _setup_spectrum_image(self, trajectory, slice_axis):
        """setup() of run_spectrum_image(): every check on the host first, then an engine of Pc <= P probes whose result ring has
        T frame slots (every frame of a probe batch is on the device when msl_tacaw runs) and whose potentials use a frame batch,
        then the detector memberships onto it"""
        if self._world > 1:
            raise NotImplementedError("spectroscopy: runs over several ranks are not supported (run_spectrum_image() is single-process)")
        if trajectory.n_frames < 2:
            raise ValueError(f"spectroscopy: TACAW needs at least 2 frames, the trajectory has {trajectory.n_frames}")
        if self._spectroscopy.segment is not None:
            from . import welch
            welch.check_segment(self._spectroscopy.segment, trajectory.n_frames, what="spectroscopy")
        from .stem_data import detector_bitmask
        dets = self._spectroscopy.detectors
        kxs, kys = self._k_axes()
        bits = detector_bitmask(dets, kxs, kys, wavelength(self.voltage_eV))
        for d, det in enumerate(dets):
            if not ((bits >> d) & 1).any():
                raise ValueError(f"detector {det.name!r} contains no stored pixel of the {len(kxs)} x {len(kys)} spectrum")
        n_slices = self._setup_run(trajectory, slice_axis)
        self._frames = list(range(self.n_frames))
        T = self.n_frames
        auto = self._probe_batch is None
        Pc = min(self.n_probes, 256 if auto else self._probe_batch)
        batch = self._frame_batch if self._frame_batch is not None else default_frame_batch(Pc, n_slices, self.nx, self.ny)
        batch = max(1, min(batch, T))
        free_b = _free_device_bytes(self.device) if auto else None
        if free_b is not None:                                  # (an explicit probe_batch is honoured as is)
            Pc = self._fit_spectrum_batch(free_b, Pc, batch)

        def shrink(Pc, slots, batch):                           # the probe batch first, then the frame batch; the ring keeps T slots
            if not auto or (Pc <= 1 and batch <= 1):
                return None
            if Pc > 1:
                Pc = max(1, Pc // 2)
            else:
                batch = max(1, batch // 2)
            logger.info(f"device memory: probe batch {Pc}, frame batch {batch}")
            return Pc, slots, batch
        self._create_engine(Pc, T, batch, shrink, device=_device_index(self.device))
        self.probe_batch = self._engine.n_probes
        self._configure_engine()                                # (the aberrations are read by the set_probes of every probe batch)
        self._engine.set_detectors(bits.reshape(-1), [d.signal for d in dets], kxs, kys)

    def _setup_run(self, trajectory, slice_axis):
        """what every engine set-up takes from the trajectory and the slice axis, stored once -> the number of slices"""
        self.base_probe = Probe(self.xs, self.ys, self.aperture, self.voltage_eV, device=self.device, aberrations=self._aberrations)
        self.n_frames = trajectory.n_frames
        self.n_probes = len(self.probe_positions)
        self.wavefunction_data = None           # filled by run(); the device holds (P,T_local,nx,ny) meanwhile
        # slice coordinates follow the slice axis (potentials.py:241-245); the Fresnel step uses zs (multislice.py:266)
        self._slice_coords = np.asarray([self.xs, self.ys, self.zs][slice_axis], dtype=np.float64)
        self._dz = self.zs[1] - self.zs[0] if self.nz > 1 else 0.5
        if getattr(self, "_projection", None) is not None:
            # the slabs are the slices: their thickness is the spacing of the slice coordinates, which must be the engine's dz
            sc = self._slice_coords
            spacing = float(sc[1] - sc[0]) if len(sc) > 1 else 0.5
            if abs(spacing - self._dz) > 1e-9 * abs(self._dz):
                raise ValueError(f"projection: slice_axis={slice_axis} gives slices {spacing:g} A thick but the propagator steps "
                                 f"{self._dz:g} A (the spacing of zs): the finite projection needs the two equal")
            self.projection_slices = self._projection.reach_slices(spacing)
            self.projection_node_spacing = spacing / self._projection.nodes
        self._Z = (atomic_numbers_of(trajectory.atom_types) if (self._generated is not None or self._absorptive is not None)
                   else np.asarray(trajectory.atom_types, dtype=np.int32))
        # A previous run's WFData (and zero-copy device views of its buffers) may still hold the old engine: drop our
        # reference and let the last owner free it, instead of closing it under them.  (A caller that keeps an earlier result
        # and only needs its host arrays frees the device side with result.release().)
        self._engine = None
        self._beam_engine = None
        return len(self._slice_coords)

    def _result_grid(self):
        """(nx, ny) of the grid the exit waves are transformed and stored on: the simulation grid, or with Prism(f, crop=True) the
        cropped one, (nx / fx, ny / fy)"""
        crop = getattr(self, "_crop", None)
        return (self.nx, self.ny) if crop is None else (self.nx // crop[0], self.ny // crop[1])

    def _source_engine(self):
        """the engine that holds the potential, the slice loop and the S-matrix: with Prism(f, crop=True) the full-grid beam engine
        (self._engine is then the result engine on the cropped grid), else the one engine of the run"""
        return self._beam_engine if getattr(self, "_beam_engine", None) is not None else self._engine

    def _stored_window(self):
        """(wx, wy) of the spectrum kept of every exit wave: the k-window, or the grid (of a cropped PRISM run: the cropped one)"""
        return self._k_window if self._k_window is not None else self._result_grid()

    def _stored_shape(self):
        """(sx, sy, pitch): the stored window divided by the detector bin, and the pixels between two images of the result (whole
        lines of 32)"""
        wx, wy = self._stored_window()
        bx, by = self._k_bin if self._k_bin is not None else (1, 1)
        return wx // bx, wy // by, ((wx // bx) * (wy // by) + 31) // 32 * 32

    def _phase_table_bytes(self, batch):
        """the phase tables of a frame group, allocated by the first potential build: up to 6 GB"""
        return min(6e9, batch * len(self.trajectory.atom_types) * (self.nx // 2 + self.ny // 2 + 2) * 8.0)

    def _stack_bytes(self):
        """device bytes per pixel, slice and frame of the batch: the two orientations of the transmission stack, and with an
        absorptive potential the two float32 stacks Vbar and Omega that its first build allocates"""
        return 24.0 if getattr(self, "_absorptive", None) is not None else 16.0

    def _fit_frame_batch(self, free_b, batch, slots):
        """Resident and streaming-TACAW runs: the default frame batch, halved while the result, the batch and what is allocated
        AFTER the engine exists -- the phase tables, the TACAW intensity array (4 B per stored complex value), the streaming
        accumulators -- exceed 0.95 x the free device memory.  A default batch that passes msl_create could otherwise run out of
        memory in the middle of a run."""
        nx, ny, n_slices = self.nx, self.ny, len(self._slice_coords)
        sx, sy, _ = self._stored_shape()
        stored = float(self.n_probes) * slots * sx * sy
        later = self._phase_table_bytes(batch) + 4.0 * stored + (24.0 * stored / slots if self._stream_tile is not None else 0.0)
        fixed = 8.0 * stored * len(self._layers) + later + 2e9        # (one result block per layer)
        per_frame = self._stack_bytes() * n_slices * nx * ny + 24.0 * nx * ny * self.n_probes
        while batch > 1 and fixed + batch * per_frame > 0.95 * free_b:
            batch = max(1, batch // 2)
        return batch

    def _fit_probe_batch(self, free_b, Pc, batch):
        """Probe-batch runs: the default probe batch, halved while the three work buffers and the result ring of Pc x batch images
        (with a thickness series also its one block, the tap buffer and the staging of every entry),
        the coherent accumulator of a split run (16 * pitch bytes per probe), the image accumulator of an imaging run (8 * nx * ny
        bytes per probe, layer and defocus), the output scratch of a polar run (8 * n_bins bytes per image), the transmission stacks
        of the batch, the TDS weight stack (4 bytes per detector, slice and pixel) and the phase tables exceed 0.9 x the free device
        memory.  With Prism(f, crop=True) the work buffers and the ring of a probe are on the cropped grid (gx, gy); the S-matrix,
        the stacks and the work buffers of the build chunk, min(Pc, Bm) beams on the beam engine, stay on the full one."""
        nx, ny, n_slices = self.nx, self.ny, len(self._slice_coords)
        gx, gy = self._result_grid()
        chunk = 32.0 * nx * ny * getattr(self, "_prism_Bm", 0) if getattr(self, "_crop", None) is not None else 0.0
        pitch = self._stored_shape()[2]
        tables = self._phase_table_bytes(batch)
        coh = 16.0 * pitch if self._diffraction is not None and self._diffraction.split else 0.0
        if getattr(self, "_dose", None) is not None:                # (the float64 frame sums and the uint32 counts of a probe's pattern)
            coh = (14.0 if getattr(self, "_camera", None) is not None else 12.0) * pitch     # (and the uint16 frames of a camera)
        if self._imaging is not None:
            coh = 8.0 * nx * ny * len(self._layers) * len(self._imaging.defocus_series)
        smatrix = 8.0 * getattr(self, "_prism_Bm", 0) * nx * ny       # the S-matrix of a PRISM run, (Bm, nx, ny) complex64
        if getattr(self, "_tds", False):                            # (a fixed cost like the S-matrix: the weight stack of every detector)
            smatrix += 4.0 * len(self._detectors) * n_slices * nx * ny
        if getattr(self, "_ionization", None) is not None:          # (the same: the weight stack and the table of every channel)
            smatrix += 4.0 * len(self._ionization) * (n_slices + 8) * nx * ny
        polar = 8.0 * self._polar.n_bins if self._polar is not None else 0.0
        series = 0.0
        if getattr(self, "_gradient", None) is not None:            # (per image the waves of every slice and the data; the accumulator once)
            series = 8.0 * n_slices * nx * ny + 4.0 * nx * ny
            smatrix += 8.0 * n_slices * nx * ny
        if self._thickness is not None and len(self._thickness) > 1:
            # the thickness series: per image one more block of the ring, the tap buffer and the detector and polar rows of every
            # entry in the float64 staging (the plain polar scratch is in `polar`); per probe the patterns of every entry
            L = len(self._thickness)
            sx, sy, _ = self._stored_shape()
            bx, by = self._diffraction.bin if self._diffraction is not None else (1, 1)
            series = 8.0 * pitch + 8.0 * nx * ny + L * polar + 8.0 * L * (len(self._detectors) if self._detectors is not None else 0)
            coh += 8.0 * L * (sx // bx) * (sy // by) if self._diffraction is not None else 0.0
        while Pc > 1 and (Pc * batch * (32.0 * gx * gy + 8.0 * pitch + polar + series) + min(chunk, 32.0 * nx * ny * Pc) + Pc * coh
                          + batch * self._stack_bytes() * n_slices * nx * ny + tables + smatrix + 1e9 > 0.9 * free_b):
            Pc = max(1, Pc // 2)
        return Pc

    def _fit_spectrum_batch(self, free_b, Pc, batch):
        """Spectrum-image runs: the default probe batch, halved while the result ring of Pc x T images and its TACAW intensity
        ((8 + 4) * pitch bytes per probe and frame), the three work buffers of Pc x batch images, the transmission stacks of the
        frame batch and the phase tables exceed 0.9 x the free device memory.  When one probe does not fit either, MemoryError: a
        smaller k_window is what shrinks the T frames of a probe."""
        nx, ny, n_slices, T = self.nx, self.ny, len(self._slice_coords), self.n_frames
        pitch = self._stored_shape()[2]
        tables = self._phase_table_bytes(batch)

        def need(Pc):
            return Pc * T * pitch * (8.0 + 4.0) + Pc * batch * 32.0 * nx * ny + batch * 16.0 * n_slices * nx * ny + tables + 1e9
        while Pc > 1 and need(Pc) > 0.9 * free_b:
            Pc = max(1, Pc // 2)
        if need(Pc) > 0.9 * free_b:
            raise MemoryError(f"spectroscopy: one probe x {T} frames of {pitch} stored pixels needs {need(1) / 1e9:.2f} GB of device memory, "
                              f"{free_b / 1e9:.2f} GB are free: keep fewer pixels with k_window=(wx, wy)")
        return Pc

    def _create_engine(self, n_probes, slots, batch, shrink, furnish=None, **engine_kw):
        """The engine of n_probes probes x slots result slots at a frame batch, then furnish(): the set-up calls that allocate on
        it.  When the device cannot hold either, shrink(n_probes, slots, batch) names the next smaller one to try, or None to
        give up."""
        while True:
            try:
                if self._crop is not None:
                    # Prism(f, crop=True): the beam engine on the full grid -- the potential, the slice loop and S; no result
                    # (n_frames = 0), and its probe count is the chunk of beams of one slice loop of smatrix_build -- and the result
                    # engine on the cropped grid, which needs no potential (one slice) and owns the ring and every reduction
                    gx, gy = self._result_grid()
                    self._beam_engine = _native.Engine(self.nx, self.ny, len(self._slice_coords), self.dx, self.dy, self._dz,
                                                       wavelength(self.voltage_eV), interaction_sigma(self.voltage_eV),
                                                       n_probes=max(1, min(n_probes, self._prism_Bm)), n_frames=0, frame_batch=1,
                                                       **{k: v for k, v in engine_kw.items() if k == "device"})
                    self._engine = _native.Engine(gx, gy, 1, self.dx, self.dy, self._dz, wavelength(self.voltage_eV),
                                                  interaction_sigma(self.voltage_eV), n_probes=n_probes, n_frames=slots,
                                                  window=self._k_window, frame_batch=1, **engine_kw)
                else:
                    self._engine = _native.Engine(self.nx, self.ny, len(self._slice_coords), self.dx, self.dy, self._dz,
                                                  wavelength(self.voltage_eV), interaction_sigma(self.voltage_eV), n_probes=n_probes,
                                                  n_frames=slots, window=self._k_window, frame_batch=batch, **engine_kw)
                if furnish is not None:
                    furnish()
                return
            except MemoryError:
                for name in ("_engine", "_beam_engine"):        # (furnish() ran out of memory: these engines go before the next)
                    if getattr(self, name) is not None:
                        getattr(self, name).close()
                        setattr(self, name, None)
                smaller = shrink(n_probes, slots, batch)
                if smaller is None:
                    raise
                n_probes, slots, batch = smaller

    def _configure_engine(self):
        eng = self._source_engine()         # (the result engine of a cropped PRISM run transforms and reduces: nothing to configure)
        eng.set_kirkland(loadKirkland())
        eng.set_slices(*slice_edges(self._slice_coords))
        eng.set_aberrations(self._aberrations)
        if self._tilt is not None and not self._tilt.is_zero:   # (no tilt: the engine keeps the tables it was created with)
            eng.set_tilt(*self._tilt.tangents)
        if self._bl_cuts is not None:                           # (no limit: no call, the tables and the builds of today)
            eng.set_bandlimit(*self._bl_cuts)
        if self._projection is not None:                        # before the first build: its tables are the channel tables
            eng.set_projection(self.projection_slices, self._projection.nodes)
        if self._absorptive is not None:                        # before the first build: its tables are f D and g
            eng.set_absorption(self._absorptive.u_by_Z, self._absorptive.absorption)
        src = self._generated
        if src is not None:                                     # the base structure, once: every build is a generation by index
            modes = isinstance(src, PhononModes)                # (the mode builds do not read the widths)
            eng.set_structure(src.positions, self._Z, np.zeros(src.n_atoms) if modes else src.sigma, self.slice_axis)
            if modes:
                eng.set_modes(src.basis_index, src.wavevectors, src.tau, src.displacements, src.dynamic)

    def _build(self, first_frame, n):
        """The potentials of the frames first_frame .. first_frame+n-1 into the batch slots (the engine's singular call at a frame
        batch of 1): MD frames from the trajectory's host array, frozen-phonon configurations and phonon-mode frames generated on
        the device by index."""
        eng = self._source_engine()
        src = self._generated
        if src is not None:
            (eng.build_modes if isinstance(src, PhononModes) else eng.build_thermal)(src.seed, first_frame, n)
        elif eng.frame_batch > 1:
            eng.build_potentials(self.trajectory.positions[first_frame:first_frame + n], self._Z, self.slice_axis)
        else:
            eng.build_potential(self.trajectory.positions[first_frame], self._Z, self.slice_axis)

    def _build_and_propagate(self, first_frame, n, first_slot, build=True, propagate=True):
        """The potentials of MD frames first_frame .. first_frame+n-1 into the batch slots, then the slice loop of every probe
        through them into result slots first_slot ..; the engine's singular calls at a frame batch of 1.  The probe-batch loops
        take the two halves apart: one build, one slice loop per probe batch."""
        eng = self._engine
        if build:
            self._build(first_frame, n)
        if propagate:
            if eng.frame_batch > 1:
                eng.propagate_frames(first_slot, n)
            else:
                eng.propagate_frame(first_slot)

    def _frame_batches(self):
        """(s0, n) per frame batch of a probe-batch run: frames s0 .. s0+n-1 go into frame slots 0 .. n-1"""
        B = self._engine.frame_batch
        return [(s0, min(B, self.n_frames - s0)) for s0 in range(0, self.n_frames, B)]

    def _members_G(self):
        """waves per scan position: the members of the Coherence, 1 without"""
        return 1 if getattr(self, "_coherence", None) is None else len(self.coherence_members[2])

    def _probe_batches(self, positions=None):
        """(p0, real, xy) per probe batch: probes p0 .. p0+real-1, and their positions (self.probe_positions, or `positions` in their
        place) padded to the engine's probe count by repeating the last one.  With a Coherence the engine's probes are waves, G per position: p0 and real count POSITIONS, a
        batch holds n_probes / G of them, and xy holds the G member positions of each, xy[q G + g] = position q + offset g"""
        G = self._members_G()
        Pc = self._engine.n_probes // G
        pos = np.asarray(self.probe_positions if positions is None else positions, dtype=np.float64).reshape(-1, 2)
        for p0 in range(0, self.n_probes, Pc):
            xy = pos[p0:p0 + Pc]
            real = len(xy)
            if real < Pc:
                xy = np.concatenate([xy, np.repeat(xy[-1:], Pc - real, axis=0)])
            if G > 1:
                xy = (xy[:, None, :] + self.coherence_members[0][None, :, :]).reshape(-1, 2)
            yield p0, real, xy

    def _set_probes(self, xy):
        """the probes of one batch of _probe_batches onto the engine: set_probes, or with a Coherence set_probe_members with the
        defocus offsets of the members repeated for every position of the batch"""
        if getattr(self, "_coherence", None) is None:
            self._engine.set_probes(self.aperture, xy)
        else:
            self._engine.set_probe_members(self.aperture, xy, np.tile(self.coherence_members[1], len(xy) // self._members_G()))

    def _detect(self, n, real):
        """(real, n, D): msl_detect of the n frames that just ran for the first `real` positions; with a Coherence the signals of
        the real x G waves, folded on the host in float64 in member order"""
        if getattr(self, "_coherence", None) is None:
            return self._engine.detect(0, n, B=real)
        from .coherence import fold_members
        return fold_members(self._engine.detect(0, n, B=real * self._members_G()), self.coherence_members[2])

    def _polar_detect(self, n, real):
        """(real, n, n_bins): msl_polar_detect likewise"""
        if getattr(self, "_coherence", None) is None:
            return self._engine.polar_detect(0, n, B=real)
        from .coherence import fold_members
        return fold_members(self._engine.polar_detect(0, n, B=real * self._members_G()), self.coherence_members[2])

    def _probe_batch_loop(self, reduce_batch):
        """The pass of run_detectors() / run_diffraction(): frame batches outside (the potentials of a batch are built once), probe
        batches inside; after the slice loop of each, reduce_batch(p0, real, s0, n) reads the engine's result ring: probes
        p0 .. p0+real-1 in its first `real` rows, frames s0 .. s0+n-1 in frame slots 0 .. n-1."""
        bar = _Progress(self._progress, self.n_frames)
        for s0, n in self._frame_batches():
            self._build_and_propagate(s0, n, 0, propagate=False)
            for p0, real, xy in self._probe_batches():
                self._set_probes(xy)
                self._build_and_propagate(s0, n, 0, build=False)
                reduce_batch(p0, real, s0, n)
            bar.update(n)
        bar.close()

    def _check_prism(self, nx, ny, world):
        """setup() of a PRISM run, before any device work: the aperture, the interpolation against the grid, one rank -> Bm"""
        fx, fy = self._prism.interpolation
        if world > 1:
            raise NotImplementedError("prism: runs over several ranks are not built (sharding of beams or probes)")
        if not self.aperture > 0:
            raise ValueError("prism needs a convergent probe: setup(aperture > 0) (a plane wave is one beam: run it without prism)")
        if nx % fx or ny % fy:
            raise ValueError(f"prism: interpolation ({fx}, {fy}) does not divide the {nx} x {ny} grid; pick a sampling whose grid it "
                             f"divides (potentials.suggest_sampling() names grid sizes near a sampling)")
        self._prism_Bm = len(prism_beams(nx, ny, self.dx, self.dy, self.aperture, wavelength(self.voltage_eV), (fx, fy)))
        if self._prism.cropped:             # (crop=True at (1, 1) runs as crop=False)
            self._crop = (fx, fy)
            if self._k_window is not None and (self._k_window[0] > nx // fx or self._k_window[1] > ny // fy):
                raise ValueError(f"prism: k_window {self._k_window} lies outside the cropped {nx // fx} x {ny // fy} spectrum of "
                                 f"Prism(({fx}, {fy}), crop=True)")

    def _prism_loop(self, reduce_batch):
        """The pass of run_detectors() / run_diffraction() with prism: per frame one potential and one S-matrix (Bm slice loops
        instead of P), then every probe batch synthesised from it into frame slot 0 and reduced as in _probe_batch_loop.  With
        Prism(f, crop=True) the S-matrix is the beam engine's and the probes go to the result engine, which reduce_batch reads."""
        eng = self._source_engine()
        bar = _Progress(self._progress, self.n_frames)
        for s in range(self.n_frames):
            self._build(s, 1)
            eng.smatrix_build()
            for p0, real, xy in self._probe_batches():
                if self._crop is not None:
                    eng.smatrix_probes_cropped(self._engine, xy, 0)
                else:
                    eng.smatrix_probes(xy, 0)
                reduce_batch(p0, real, s, 1)
            bar.update(1)
        bar.close()

    def _frames_inside_loop(self, reduce_batch, finish_batch, coherent=True, own_slots=False):
        """The other loop order, for the elastic / thermal-diffuse split of run_diffraction(): probe batches outside, frame batches
        inside, because |<Psi>|^2 needs the coherent sum over ALL frames of a probe while its accumulator (16 * pitch bytes per
        probe) is on the device.  Per probe batch: set_probes once (a potential build leaves the probes alone), coherent_reset;
        per frame batch inside it the potentials, the slice loop, reduce_batch(p0, real, s0, n) as in _probe_batch_loop and
        coherent_add of the n new frames; then finish_batch(p0, real).  The price: the potentials of every frame are built once
        per probe batch, ceil(P / Pc) times instead of once -- except when the whole trajectory is one frame batch, which is
        built once before the probe loop.  run_images() takes the same order with coherent=False (its accumulator holds one probe
        batch too): no coherent_* call is made.  own_slots=True (run_spectrum_image(), whose ring has a slot for every frame): frame
        batch s0 goes to result slots s0 .. s0+n-1 instead of 0 .. n-1, so that all T frames of the probe batch are in the ring when
        finish_batch runs."""
        eng, batches = self._engine, self._frame_batches()
        bar = _Progress(self._progress, -(-self.n_probes // (eng.n_probes // self._members_G())) * self.n_frames)
        once = self.n_frames <= eng.frame_batch
        if once:
            self._build_and_propagate(0, self.n_frames, 0, propagate=False)
        for p0, real, xy in self._probe_batches():
            self._set_probes(xy)
            if coherent:
                eng.coherent_reset()
            for s0, n in batches:
                self._build_and_propagate(s0, n, s0 if own_slots else 0, build=not once)
                reduce_batch(p0, real, s0, n)
                if coherent:
                    eng.coherent_add(0, n, B=real)
                bar.update(n)
            finish_batch(p0, real)
        bar.close()

    def _stem_data(self, signals, tds_per_slice=None):
        from .stem_data import STEMData
        kxs, kys = self._k_axes()
        return self._tag_crop(STEMData(signals=signals, detectors=list(self._detectors), probe_positions=self.probe_positions,
                                       time=np.arange(self.n_frames) * self.trajectory.timestep, kxs=_as_tensor(kxs), kys=_as_tensor(kys),
                                       probe=self.base_probe, tds_per_slice=tds_per_slice, coherence=getattr(self, "_coherence", None),
                                       **self._layer_fields()))

    def _tag_crop(self, result):
        """a result of a Prism(f, crop=True) run carries .prism_crop = (fx, fy): its pixels are the uncropped run's at
        prism.crop_index, not rescaled, on the cropped grid's own k axes"""
        if self._crop is not None:
            result.prism_crop = self._crop
        return result

    def _layer_fields(self):
        """layer / thickness of a result with a thickness axis: the slice indices, and the depth in Angstrom at the exit side of each
        slice, from the slice edges the engine was given"""
        if self._thickness is None:
            return {}
        lo, hi = slice_edges(self._slice_coords)
        ks = np.asarray(self._thickness, dtype=np.int64)
        return dict(layer=ks, thickness=hi[ks] - lo[0])

    def _layered(self, shape):
        """host result of `shape`, with the thickness axis last when there is one"""
        return np.zeros(shape + ((len(self._thickness),) if self._thickness is not None else ()), dtype=np.float64)

    def _position_batch(self, acc, p0, real, n, want_det):
        """run_diffraction() with a thickness series, one probe batch: the patterns of every entry, summed over the n frames, into
        rows p0 .. of acc (P, mx, my, L) -> the detector signals (L, real, n, D) of the same fetch, or None"""
        det, _, pat = self._layer_signals(real, n)
        acc[p0:p0 + real] += np.moveaxis(pat, 0, -1)
        return det

    def _pacbed_batch(self, acc, p0, real, n, want_det):
        """The same with patterns="pacbed", acc (mx, my, L): the device sums the patterns over the probes of a frame batch -- reset
        before its first probe batch, one add per probe batch, one download after its last -- and the host adds the frame batches.
        The fetch is made for the detector signals only.  (The exit wave alone has no accumulator: its patterns are summed here.)"""
        eng = self._engine
        if len(self._thickness) == 1:
            det, _, pat = self._layer_signals(real, n)
            acc += np.moveaxis(pat.sum(axis=1), 0, -1)
            return det
        if p0 == 0:
            eng.layer_pacbed_reset()
        eng.layer_pacbed_add(real)
        if p0 + real == self.n_probes:
            acc += np.moveaxis(eng.layer_pacbed(), 0, -1)
        return self._layer_signals(real, n)[0] if want_det else None

    def _layer_signals(self, real, n):
        """(det, polar, patterns) of the slice loop that just ran n frames, for the first `real` probes and every thickness entry:
        (L, real, n, D), (L, real, n, n_bins), (L, real, mx, my), None for what the run does not form (and for the patterns of a
        pacbed run, which stay on the device).  One fetch; the exit wave alone (L = 1) has no tap and takes the plain reductions."""
        eng = self._engine
        if len(self._thickness) > 1:
            return eng.layer_fetch(n, B=real)
        return (None if self._detectors is None else eng.detect(0, n, B=real)[None],
                None if self._polar is None else eng.polar_detect(0, n, B=real)[None],
                None if self._diffraction is None else eng.diffract(0, n, B=real, bin=self._diffraction.bin)[None])

    def _precess(self, run, fields):
        """A precession run: one scan `run()` per tilt of the cone, the engine's tables rewritten in between (msl_set_tilt is ordered
        on the stream behind the scan before it) -> the result of the last scan with every array named in `fields` (and the signals
        of its .stem) replaced by the mean over the tilts, added in float64 in tilt order, and the tilts in .tilts"""
        tilts = self._precession.tilts()
        t0 = time.time()
        sums, out = {}, None
        self._precessing = True
        try:
            for t in tilts:
                self._source_engine().set_tilt(*t.tangents)
                out = run()
                for owner, name in [(out, f) for f in fields] + ([(out.stem, "signals")] if getattr(out, "stem", None) is not None else []):
                    val = getattr(owner, name)
                    if val is None:
                        continue
                    key = (owner is out, name)
                    if key in sums:
                        sums[key] += val
                    else:
                        sums[key] = np.array(val, dtype=np.float64)
        finally:
            self._precessing = False
        for (top, name), total in sums.items():
            setattr(out if top else out.stem, name, total / len(tilts))
        out.tilts = tilts
        if getattr(out, "stem", None) is not None:
            out.stem.tilts = tilts
        self.elapsed = time.time() - t0
        return out

    def run_diffraction(self):
        """Frame-averaged diffraction pattern of every probe position (4D-STEM / CBED): the loop of run_detectors(); msl_diffract
        reduces the exit spectra of every probe batch to (real, mx, my) float64 -- |Psi|^2 summed over the frames of the batch and
        the pixels of each bin -- which is added into the host result and divided by the number of frames at the end.
        -> DiffractionData with intensity (P, mx, my) float64; with detectors as well, .stem is the STEMData run_detectors()
        returns, from the same propagation.  Device memory does not depend on the number of probe positions; the host holds
        8 * P * mx * my bytes (537 MB for 64 x 64 positions x 128 x 128 detector pixels), which is not checked against anything.
        With Diffraction(split=True) the result also carries `elastic`, |<Psi>|^2 summed over each bin (and .tds, .part()): the
        run then takes the other loop order (_frames_inside_loop: probe batches outside, every frame of a probe added into a
        float64 accumulator on the device), which builds the potentials of every frame once per probe batch instead of once, and
        the host holds a second (P, mx, my) array.  intensity and stem are computed by the same calls as without the split.
        With Diffraction(dose=Dose(...)) the run takes that loop order too: per probe batch msl_dose_reset, per frame batch
        msl_dose_add (the pattern pass, added into the float64 accumulator on the device), then msl_dose_counts draws the Poisson
        counts there (dose.py) and downloads 4 bytes per detector pixel -> .counts (P, mx, my) uint32; .intensity only with
        Dose(keep_intensity=True).  The counts do not depend on probe_batch (the draws are keyed by the
        probe's index in the scan).
        With Diffraction(dose=..., camera=Camera(...)) msl_dose_frames takes the place of msl_dose_counts: the draw, then the camera's
        response to the counts on the device (camera.py), and 2 bytes per detector pixel downloaded -> .frames (P, mx, my) uint16;
        .counts only with Camera(keep_counts=True).  The readout noise is keyed as the draws are: no dependence on probe_batch."""
        from .diffraction_data import DiffractionData, bin_centres
        if self._spectroscopy is not None:
            raise RuntimeError("spectroscopy is set: the device holds one probe batch at a time -- call run_spectrum_image()")
        if self._diffraction is None:
            raise RuntimeError("run_diffraction() needs MultisliceCalculator(diffraction=Diffraction(...))")
        if self._engine is None:
            raise RuntimeError("call setup() before run_diffraction()")
        if self._precession is not None and not self._precessing:
            return self._precess(self.run_diffraction, ('intensity', 'elastic'))
        eng = self._engine
        t0 = time.time()
        P, T = self.n_probes, self.n_frames
        bx, by = self._diffraction.bin
        pacbed = self._thickness is not None and self._thickness_arg.patterns == "pacbed"
        dose = self._dose
        members = None if getattr(self, "_coherence", None) is None else self.coherence_members
        mx, my = eng.wx // bx, eng.wy // by
        keep = dose is None or dose.keep_intensity
        acc = self._layered(((mx, my) if pacbed else (P, mx, my)) if keep else (0,))
        signals = None if self._detectors is None else self._layered((P, T, len(self._detectors)))
        counts = incident = frames = None
        camera = self._camera
        if dose is not None:
            from .dose import incident_intensity
            if camera is None or camera.keep_counts:
                counts = np.zeros((P, mx, my), dtype=np.uint32)
            if camera is not None:
                frames = np.zeros((P, mx, my), dtype=np.uint16)
                eng.set_camera(camera)
            incident = incident_intensity(self.nx, self.ny, self.dx, self.dy, self.aperture, wavelength(self.voltage_eV))
            dose_scale = self.electrons_per_probe / (T * incident)      # electrons per unit of the frame SUM

        def reduce_batch(p0, real, s0, n):
            if dose is not None:                                # the frame sums stay on the device until finish_batch
                if s0 == 0:
                    eng.dose_reset(real, (mx, my))
                if members is None:
                    eng.dose_add(0, n, B=real, bin=(bx, by))
                else:                                           # (the G member patterns of a position, folded into its one row)
                    eng.dose_add_members(members[2], 0, n, B=real * len(members[2]), bin=(bx, by))
                if signals is not None:
                    signals[p0:p0 + real, s0:s0 + n] = self._detect(n, real)
                return
            if self._thickness is not None:
                det = (self._pacbed_batch if pacbed else self._position_batch)(acc, p0, real, n, signals is not None)
                if signals is not None:
                    signals[p0:p0 + real, s0:s0 + n] = np.moveaxis(det, 0, -1)
                return
            if members is None:
                acc[p0:p0 + real] += eng.diffract(0, n, B=real, bin=(bx, by))
            else:
                acc[p0:p0 + real] += eng.diffract_members(members[2], 0, n, B=real * len(members[2]), bin=(bx, by))
            if signals is not None:
                signals[p0:p0 + real, s0:s0 + n] = self._detect(n, real)
        elastic = None
        if self._diffraction.split:
            elastic = np.zeros_like(acc)

            def finish_batch(p0, real):
                elastic[p0:p0 + real] = eng.coherent_finish(T, B=real, bin=(bx, by))
            self._frames_inside_loop(reduce_batch, finish_batch)
        elif dose is not None:
            def finish_batch(p0, real):
                if camera is not None:
                    frames[p0:p0 + real], cnt, sums = eng.dose_frames(dose_scale, dose.seed, probe0=p0, B=real,
                                                                      keep_counts=camera.keep_counts, keep_intensity=keep)
                    if cnt is not None:
                        counts[p0:p0 + real] = cnt
                else:
                    counts[p0:p0 + real], sums = eng.dose_counts(dose_scale, dose.seed, probe0=p0, B=real, keep_intensity=keep)
                if keep:
                    acc[p0:p0 + real] = sums
            self._frames_inside_loop(reduce_batch, finish_batch, coherent=False)
        elif self._prism is not None:
            self._prism_loop(reduce_batch)
        else:
            self._probe_batch_loop(reduce_batch)
        acc /= (P * T) if pacbed else T
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        kxs, kys = self._k_axes()
        return self._tag_crop(DiffractionData(intensity=acc if keep else None, kxs=_as_tensor(bin_centres(kxs, bx)),
                                              kys=_as_tensor(bin_centres(kys, by)),
                                              bin=(bx, by), n_frames=T, probe_positions=self.probe_positions, probe=self.base_probe,
                                              stem=None if signals is None else self._stem_data(signals), elastic=elastic,
                                              patterns="pacbed" if pacbed else "position", counts=counts, dose=dose,
                                              electrons_per_probe=self.electrons_per_probe if dose is not None else None,
                                              incident=incident, frames=frames, camera=camera, coherence=getattr(self, "_coherence", None),
                                              **self._layer_fields()))

    def run_gradient(self, data, frame=0, potential=None, positions=None, probe_positions=None, aberrations=None):
        """The derivative of the data-fit loss of MultisliceCalculator(gradient=Gradient(...)) with respect to the slice potentials
        (adjoint.py is the definition): per probe batch msl_adjoint_add runs the forward loop, which keeps the wave arriving at every
        slice, the residual of the exit patterns against `data` and the loop backwards, and adds into a float64 accumulator on the
        device (no atomics: repeats give the same bits; another probe_batch changes the order of the float64 sums only).
        data: (P, nx, ny) in the layout and units of DiffractionData.intensity of an unbinned, unwindowed run, or such a
        DiffractionData.  frame: the trajectory frame whose potential is built.  potential: (nx, ny, nz) -- the caller's estimate,
        uploaded in place of the build (what an iterative reconstruction passes at every step).  positions: (n_atoms, 3) -- the
        caller's current coordinates, built in place of the trajectory frame (what a structure refinement passes at every step).
        With Gradient(positions=True) the chain goes on through the potential build (msl_adjoint_positions, on the accumulator and
        the phase tables the build left on the device): GradientData.positions is dL/dr_a, (n_atoms, 3) float64, the slice-axis
        column zero.  potential= has no atoms: ValueError with positions= or with Gradient(positions=True).
        With Gradient(probe_positions=True) / Gradient(aberrations=True) the chain also goes back through the probe recipe
        (msl_adjoint_probe_params per batch, on the probe gradient msl_adjoint_add left on the device):
        GradientData.probe_position_gradient is dL/d(x_p, y_p), (P, 2) float64 per Angstrom, and .aberration_gradient maps the names of
        the Aberrations fields to dL/dC_nm per Angstrom and dL/dphi_nm per radian (section 4.33).  probe_positions: (P, 2) scan
        positions and aberrations: an Aberrations, in place of those of setup() for this call (what a refinement passes at every
        step); the engine's aberrations are put back afterwards, so a later run is what it was.  -> GradientData."""
        from .gradient_data import GradientData
        grad = getattr(self, "_gradient", None)
        if grad is None:
            raise RuntimeError("run_gradient() needs MultisliceCalculator(gradient=Gradient(...))")
        if self._engine is None:
            raise RuntimeError("call setup() before run_gradient()")
        eng = self._engine
        if hasattr(data, "intensity"):
            if tuple(getattr(data, "bin", (1, 1))) != (1, 1):
                raise ValueError("gradient: the data must be unbinned patterns (Diffraction(bin=(1, 1)))")
            data = data.intensity
        data = np.asarray(data.detach().cpu().numpy() if hasattr(data, "detach") else data)
        nz = len(self._slice_coords)
        if data.shape != (self.n_probes, self.nx, self.ny):
            raise ValueError(f"gradient: data {data.shape} does not match ({self.n_probes}, {self.nx}, {self.ny}): the unbinned, unwindowed "
                             "pattern of every probe position")
        if not 0 <= int(frame) < self.n_frames:
            raise ValueError(f"gradient: frame {frame} outside [0, {self.n_frames})")
        if potential is not None and positions is not None:
            raise ValueError("gradient: potential= and positions= are two sources of the same stack: pass one")
        if potential is not None and grad.positions:
            raise ValueError("gradient: Gradient(positions=True) differentiates the potential build, and potential= does not come from atoms")
        if positions is not None:
            positions = np.ascontiguousarray(positions, dtype=np.float64)
            if positions.shape != (len(self._Z), 3) or not np.isfinite(positions).all():
                raise ValueError(f"gradient: positions {positions.shape} must be finite ({len(self._Z)}, 3) coordinates, one row per atom")
        if grad.probe_params and not self.aperture > 0:
            raise NotImplementedError("gradient: probe_positions / aberrations of plane-wave illumination (aperture=0) is not built")
        scan = np.asarray(self.probe_positions, dtype=np.float64).reshape(-1, 2)
        if probe_positions is not None:
            try:
                scan = np.ascontiguousarray(probe_positions, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"gradient: probe_positions must be ({self.n_probes}, 2) finite scan positions") from None
            if scan.shape != (self.n_probes, 2) or not np.isfinite(scan).all():
                raise ValueError(f"gradient: probe_positions {scan.shape} must be finite ({self.n_probes}, 2) scan positions, one row per probe")
        if aberrations is not None and not isinstance(aberrations, Aberrations):
            raise ValueError(f"gradient: aberrations: expected an Aberrations object, got {aberrations!r}")
        lens = self._aberrations if aberrations is None else aberrations
        t0 = time.time()
        if potential is not None:
            V = np.asarray(potential)
            if V.shape != (self.nx, self.ny, nz):
                raise ValueError(f"gradient: potential {V.shape} does not match ({self.nx}, {self.ny}, {nz})")
            eng.upload_potential(np.ascontiguousarray(np.moveaxis(V, 2, 0), dtype=np.float32))
        elif positions is not None:
            eng.build_potential(positions, self._Z, self.slice_axis)
        else:
            self._build(int(frame), 1)
        eng.adjoint_reset()
        loss = np.zeros(self.n_probes, dtype=np.float64)
        probe = np.zeros((self.n_probes, self.nx, self.ny), dtype=np.complex64) if grad.probe else None
        params = np.zeros((self.n_probes, 30), dtype=np.float64) if grad.probe_params else None
        if aberrations is not None:
            eng.set_aberrations(aberrations)
        try:
            for p0, real, xy in self._probe_batches(None if probe_positions is None else scan):
                self._set_probes(xy)
                l, pg = eng.adjoint_add(data[p0:p0 + real], B=real, probe=grad.probe)
                loss[p0:p0 + real] = l
                if probe is not None:
                    probe[p0:p0 + real] = pg
                if params is not None:
                    params[p0:p0 + real] = eng.adjoint_probe_params(B=real)
        finally:
            if aberrations is not None:
                eng.set_aberrations(self._aberrations)
        g = np.ascontiguousarray(np.moveaxis(eng.adjoint_download(), 0, 2))
        pos_grad = eng.adjoint_positions() if grad.positions else None
        self.elapsed = time.time() - t0
        extra = {}
        if params is not None:
            from .adjoint import aberration_polar_gradient
            from .aberrations import TERMS
            if grad.probe_positions:
                extra["probe_position_gradient"] = np.ascontiguousarray(params[:, :2])
            if grad.aberrations:
                cart = params[:, 2:].sum(axis=0).reshape(14, 2)
                dC, dphi = aberration_polar_gradient(cart, lens, wavelength(self.voltage_eV))
                named = {}
                for j, (name, n, m) in enumerate(TERMS):
                    named[name] = float(dC[j])
                    if m:
                        named["phi" + name[1:]] = float(dphi[j])
                extra.update(aberration_gradient=named, aberration_gradient_cartesian=cart)
        return GradientData(potential=g, loss=loss, sigma=interaction_sigma(self.voltage_eV), xs=self.xs, ys=self.ys, zs=self._slice_coords,
                            probe=probe, kind=grad.loss, frame=int(frame),
                            probe_positions=self.probe_positions if probe_positions is None else scan, positions=pos_grad, **extra)

    def run_images(self):
        """Frame-averaged images behind the objective lens (HRTEM, focal series), for every probe: probe batches outside, frame
        batches inside (_frames_inside_loop without its coherent sums), because the float64 accumulator on the device,
        (real, L, F, nx, ny), holds one probe batch.  Per probe batch it is reset; per frame batch, after the slice loop, one
        msl_image_add for every defocus f and focal-spread node i (weight w_i, image l * F + f of every probe, stride L * F) applies
        the lens to the n new exit spectra, transforms back and adds |psi|^2; after the last frame batch the images are downloaded
        and divided by the number of frames.  -> ImageData with intensity (P, L, F, nx, ny) float64, L = 1.  As for the split of
        run_diffraction(), the potentials of every frame are built once per probe batch unless the trajectory is one frame batch."""
        from .image_data import ImageData
        if self._spectroscopy is not None:
            raise RuntimeError("spectroscopy is set: the device holds one probe batch at a time -- call run_spectrum_image()")
        if self._imaging is None:
            raise RuntimeError("run_images() needs MultisliceCalculator(imaging=Imaging(...))")
        if self._engine is None:
            raise RuntimeError("call setup() before run_images()")
        eng, im = self._engine, self._imaging
        t0 = time.time()
        P, T, L, F = self.n_probes, self.n_frames, len(self._layers), len(im.defocus_series)
        lam = wavelength(self.voltage_eV)
        k_ap = im.aperture_k(lam)
        deltas, weights = im.nodes()
        polars = [[im.polar(f, i) for i in range(len(deltas))] for f in range(F)]
        out = np.zeros((P, L, F, eng.wx, eng.wy), dtype=np.float64)       # (imaging stores the full grid: wx, wy = nx, ny)

        def reduce_batch(p0, real, s0, n):
            if s0 == 0:
                eng.image_reset(real * L * F)
            for f in range(F):
                for i, w in enumerate(weights):
                    eng.image_add(0, n, polar=polars[f][i], aperture_k=k_ap, weight=float(w), first=(L - 1) * F + f, stride=L * F, B=real)

        def finish_batch(p0, real):
            out[p0:p0 + real] = np.asarray(eng.image_download(0, real * L * F)).reshape(real, L, F, eng.wx, eng.wy) / T
        self._frames_inside_loop(reduce_batch, finish_batch, coherent=False)
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        return ImageData(intensity=out, xs=np.asarray(self.xs, dtype=np.float64), ys=np.asarray(self.ys, dtype=np.float64),
                         defocus=np.asarray(im.defocus_series, dtype=np.float64), layer=np.asarray(self._layers, dtype=np.int64),
                         n_frames=T, probe_positions=self.probe_positions, imaging=im)

    def run_spectrum_image(self):
        """Energy-resolved detector signals of every probe position: probe batches outside, frame batches inside
        (_frames_inside_loop), because the time transform needs ALL frames of a probe.  Per probe batch: set_probes once; per frame
        batch the potentials and the slice loop into the ring's frame slots s0 ..; then msl_tacaw turns the (Pc, T, pitch) ring into
        its intensity, | fftshift_t fft_t(Psi - <Psi>_t) |^2 (tacaw_data.py:89-104; the zero-frequency bin is zero), and ONE
        msl_spectrum_detect pass sums it over the stored pixels of every detector -> rows p0 .. p0+real-1 of the result.  With
        Spectroscopy(stem=True) msl_detect reads the same ring for the per-frame signals run_detectors() returns.
        With Spectroscopy(segment=L) msl_tacaw_welch takes msl_tacaw's place and the spectra have L bins.
        -> SpectrumImageData with spectra (P, T, D) float64 ((P, L, D) with a segment).  Device memory does not depend on the number of probe positions.  As for
        the split of run_diffraction(), the potentials of every frame are built once per probe batch, ceil(P / Pc) times instead of
        once, unless the whole trajectory is one frame batch, which is built once before the probe loop."""
        from .spectrum_image_data import SpectrumImageData
        if self._spectroscopy is None:
            raise RuntimeError("run_spectrum_image() needs MultisliceCalculator(spectroscopy=Spectroscopy(...))")
        if self._engine is None:
            raise RuntimeError("call setup() before run_spectrum_image()")
        eng, dets = self._engine, self._spectroscopy.detectors
        sp = self._spectroscopy
        t0 = time.time()
        P, T, D = self.n_probes, self.n_frames, len(dets)
        F = T if sp.segment is None else sp.segment             # (segment=L: Welch's estimate, L frequency bins; msl_tacaw_welch)
        spectra = np.zeros((P, F, D), dtype=np.float64)
        signals = np.zeros((P, T, D), dtype=np.float64) if self._spectroscopy.stem else None

        def reduce_batch(p0, real, s0, n):                      # (nothing per frame batch: the transform needs every frame)
            pass

        def finish_batch(p0, real):
            if sp.segment is None:
                eng.tacaw()
            else:
                eng.tacaw_welch(sp.segment, sp.hop, sp.window)
            spectra[p0:p0 + real] = eng.spectrum_detect(B=real)
            if signals is not None:
                signals[p0:p0 + real] = eng.detect(0, T, B=real)
        self._frames_inside_loop(reduce_batch, finish_batch, coherent=False, own_slots=True)
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        stem = None
        if signals is not None:
            from .stem_data import STEMData
            kxs, kys = self._k_axes()
            stem = STEMData(signals=signals, detectors=list(dets), probe_positions=self.probe_positions,
                            time=np.arange(T) * self.trajectory.timestep, kxs=_as_tensor(kxs), kys=_as_tensor(kys), probe=self.base_probe)
        freqs = np.fft.fftshift(np.fft.fftfreq(F, d=self.trajectory.timestep))
        return SpectrumImageData(spectra=spectra, frequencies=freqs, detectors=list(dets), probe_positions=self.probe_positions,
                                 n_frames=T, stem=stem)

    def run_detectors(self):
        """STEM detector signals of every probe and frame: for each frame batch the potentials are built once, then every probe
        batch goes through the slice loop and msl_detect reduces its exit spectra to the detector values.  -> STEMData with
        signals (P, T, D) float64."""
        if self._spectroscopy is not None:
            raise RuntimeError("spectroscopy is set: the device holds one probe batch at a time -- call run_spectrum_image()")
        if self._engine is None:
            raise RuntimeError("call setup() before run_detectors()")
        if self._detectors is None and self._polar is not None:
            raise RuntimeError("polar is set and detectors are not: call run_polar()")
        if self._detectors is None:
            raise RuntimeError("run_detectors() needs MultisliceCalculator(detectors=[...])")
        if self._precession is not None and not self._precessing:
            return self._precess(self.run_detectors, ('signals',))
        eng = self._engine
        t0 = time.time()
        P, T, D = self.n_probes, self.n_frames, len(self._detectors)
        signals = self._layered((P, T, D))
        tds = np.zeros((P, T, D, len(self._slice_coords)), dtype=np.float64) if self._tds else None

        def reduce_batch(p0, real, s0, n):
            if tds is not None:
                # (nz, real, D) of the slice loop that just ran, one frame, in the units of `signals`: the exit FFT is unnormalised,
                # sum_k |Psi|^2 = nx ny sum_r |psi|^2
                tds[p0:p0 + real, s0] = np.moveaxis(eng.tds_fetch(B=real), 0, -1) * float(self.nx * self.ny)
            if self._thickness is not None:
                signals[p0:p0 + real, s0:s0 + n] = np.moveaxis(self._layer_signals(real, n)[0], 0, -1)
                return
            signals[p0:p0 + real, s0:s0 + n] = self._detect(n, real)
        if self._prism is not None:
            self._prism_loop(reduce_batch)
        else:
            self._probe_batch_loop(reduce_batch)
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        return self._stem_data(signals, tds)

    def run_element_maps(self):
        """Element maps (ionization.py is the definition): the loop of run_detectors() at a frame batch of 1 -- per frame the
        potential and with it the weight stack of every channel, then every probe batch through the two-pass slice loop, which
        reduces |psi|^2 against the weights slice by slice (msl_set_ionization); the sums of every frame are fetched and added on
        the host in float64 and divided by the number of frames.  -> ElementMapData with per_slice (P, E, nz)."""
        if self._ionization is None:
            raise RuntimeError("run_element_maps() needs MultisliceCalculator(ionization=[Ionization(...), ...])")
        if self._engine is None:
            raise RuntimeError("call setup() before run_element_maps()")
        from .element_map_data import ElementMapData
        eng = self._engine
        t0 = time.time()
        P, T, E = self.n_probes, self.n_frames, len(self._ionization)
        per_slice = np.zeros((P, E, len(self._slice_coords)), dtype=np.float64)

        def reduce_batch(p0, real, s0, n):
            per_slice[p0:p0 + real] += np.moveaxis(eng.ionization_fetch(B=real), 0, -1)      # (nz, real, E) of the frame that just ran
        self._probe_batch_loop(reduce_batch)
        per_slice /= float(T)
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        lo, hi = slice_edges(self._slice_coords)
        return ElementMapData(per_slice=per_slice, channels=list(self._ionization), probe_positions=self.probe_positions,
                              thickness=hi - lo[0], n_frames=T)

    def run_polar(self):
        """Polar-detector signals of every probe position: the loop of run_detectors(); msl_polar_detect reduces the exit spectra of
        every probe batch to (real, n, R * A) float64 -- |Psi|^2 summed over the pixels of each ring x sector bin, frame by frame --
        which is stored (PolarDetector(per_frame=True)) or summed over the n frames into the host result and divided by the number of
        frames at the end.  -> PolarData with signals (P, R, A) float64, (P, T, R, A) per frame; with detectors as well, .stem is
        the STEMData run_detectors() returns, from the same propagation.  Device memory does not depend on the number of probe
        positions; the host holds 8 * P * R * A bytes (times T per frame)."""
        from .polar_data import PolarData
        if self._spectroscopy is not None:
            raise RuntimeError("spectroscopy is set: the device holds one probe batch at a time -- call run_spectrum_image()")
        if self._polar is None:
            raise RuntimeError("run_polar() needs MultisliceCalculator(polar=PolarDetector(...))")
        if self._engine is None:
            raise RuntimeError("call setup() before run_polar()")
        if self._precession is not None and not self._precessing:
            return self._precess(self.run_polar, ('signals',))
        eng, pol = self._engine, self._polar
        t0 = time.time()
        P, T, R, A = self.n_probes, self.n_frames, pol.n_rings, pol.n_azimuthal
        acc = self._layered((P, T, R * A) if pol.per_frame else (P, R * A))
        signals = None if self._detectors is None else self._layered((P, T, len(self._detectors)))

        def reduce_batch(p0, real, s0, n):
            if self._thickness is not None:
                det, got, _ = self._layer_signals(real, n)
                got = np.moveaxis(got, 0, -1)                   # (real, n, R * A, L)
                if pol.per_frame:
                    acc[p0:p0 + real, s0:s0 + n] = got
                else:
                    acc[p0:p0 + real] += got.sum(axis=1)
                if signals is not None:
                    signals[p0:p0 + real, s0:s0 + n] = np.moveaxis(det, 0, -1)
                return
            got = self._polar_detect(n, real)
            if pol.per_frame:
                acc[p0:p0 + real, s0:s0 + n] = got
            else:
                acc[p0:p0 + real] += got.sum(axis=1)
            if signals is not None:
                signals[p0:p0 + real, s0:s0 + n] = self._detect(n, real)
        if self._prism is not None:
            self._prism_loop(reduce_batch)
        else:
            self._probe_batch_loop(reduce_batch)
        if not pol.per_frame:
            acc /= T
        self.elapsed = time.time() - t0
        self.frames_computed, self.frames_cached = T, 0
        kxs, kys = self._k_axes()
        if self._thickness is not None:
            acc = acc.reshape(acc.shape[:-2] + (R, A, acc.shape[-1]))
        else:
            acc = acc.reshape(acc.shape[:-1] + (R, A))
        return self._tag_crop(PolarData(signals=acc, polar=pol, counts=self._polar_counts.reshape(R, A), edges=pol.edges,
                                        probe_positions=self.probe_positions, time=np.arange(T) * self.trajectory.timestep,
                                        kxs=_as_tensor(kxs), kys=_as_tensor(kys), probe=self.base_probe,
                                        stem=None if signals is None else self._stem_data(signals), coherence=getattr(self, "_coherence", None),
                                        **self._layer_fields()))

    def _check_layers(self, n_slices, world):
        """the `layers` argument -> sorted unique slice indices with n_slices - 1 last (before any device work)"""
        if self._layers_arg is None:
            return [n_slices - 1]
        if world > 1:
            raise NotImplementedError("layers: runs over several ranks gather the exit wave only")
        out = set()
        for k in self._layers_arg:
            if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
                raise ValueError(f"layers must be integer slice indices, got {k!r}")
            if not 0 <= int(k) <= n_slices - 1:
                raise ValueError(f"layer slice index {k} outside [0, {n_slices - 1}]")
            out.add(int(k))
        out.discard(n_slices - 1)
        return sorted(out) + [n_slices - 1]

    def _check_layer_memory(self, dev, slots):
        """L result blocks (P, T_local, pitch) c64 must fit in the device's free memory: fail before anything is allocated"""
        L = len(self._layers)
        free_b = None if L == 1 else _free_device_bytes(dev)
        if free_b is None:                                  # (the exit wave only, or no device visible: msl_set_layers decides)
            return
        need = 8.0 * L * self.n_probes * slots * self._stored_shape()[2]
        if need > free_b:
            raise MemoryError(f"layers: {L} layers of {self.n_probes} probes x {slots} frames need {need / 1e9:.1f} GB of device memory, "
                              f"{free_b / 1e9:.1f} GB are free")

    def run(self) -> WFData:
        """reference calculators.py:163-250: all frames, then pack WFData."""
        if getattr(self, "_coherence", None) is not None:
            raise NotImplementedError("coherence: run() is not built (a partially coherent probe has no single exit wave): call "
                                      "run_detectors(), run_polar() or run_diffraction()")
        if self._detectors is not None:
            raise RuntimeError("detectors are set: the device holds one probe batch at a time -- call run_detectors()")
        if self._diffraction is not None:
            raise RuntimeError("diffraction is set: the device holds one probe batch at a time -- call run_diffraction()")
        if self._imaging is not None:
            raise RuntimeError("imaging is set: the device holds one probe batch at a time -- call run_images()")
        if self._spectroscopy is not None:
            raise RuntimeError("spectroscopy is set: the device holds one probe batch at a time -- call run_spectrum_image()")
        if self._polar is not None:
            raise RuntimeError("polar is set: the device holds one probe batch at a time -- call run_polar()")
        if self._ionization is not None:
            raise RuntimeError("ionization is set: the device holds one probe batch at a time -- call run_element_maps()")
        if self._engine is None:
            raise RuntimeError("call setup() before run()")
        if self._stream_tile is not None:
            raise RuntimeError("stream_tile is set: the device holds a ring of frames only -- call run_streaming_tacaw()")
        eng = self._engine
        t0 = time.time()
        frames = self._frames
        bar = _Progress(self._progress and self._rank == 0, len(frames))
        self.frames_computed = self.frames_cached = 0
        if self._cache:
            # frame by frame (setup() gave the engine a frame batch of 1): a frame found in the cache is loaded, the others are written
            for slot, frame_idx in enumerate(frames):
                cache_file = self.output_dir / f"frame_{frame_idx}.npy"
                if cache_file.exists():
                    eng.upload_frame(slot, np.load(cache_file)[:, :, :, 0, 0])
                    self.frames_cached += 1
                else:
                    self._build(frame_idx, 1)
                    eng.propagate_frame(slot)
                    self.frames_computed += 1
                    np.save(cache_file, eng.frame(slot).astype(np.complex128)[:, :, :, None, None])
                bar.update(1)
        elif self._prism is not None:
            # per frame: the potential, the S-matrix of its Bm beams, every probe synthesised from it into the frame's slot
            xy = np.asarray(self.probe_positions, dtype=np.float64).reshape(-1, 2)
            src = self._source_engine()      # (Prism(f, crop=True): the beam engine; eng is the result engine on the cropped grid)
            for slot, frame_idx in enumerate(frames):
                self._build(frame_idx, 1)
                src.smatrix_build()
                if self._crop is not None:
                    src.smatrix_probes_cropped(eng, xy, slot)
                else:
                    src.smatrix_probes(xy, slot)
                self.frames_computed += 1
                bar.update(1)
        else:
            # batches of B frames: B potentials into the batch slots, then one slice loop over B x P images
            for s0 in range(0, len(frames), eng.frame_batch):
                chunk = frames[s0:s0 + eng.frame_batch]          # (a rank's frames are one contiguous block)
                self._build_and_propagate(chunk[0], len(chunk), s0)
                self.frames_computed += len(chunk)
                bar.update(len(chunk))
        eng.synchronize()
        bar.close()
        self.elapsed = time.time() - t0
        logger.info(f"Simulation completed in {self.elapsed:.2f}s ({self.frames_computed} computed, {self.frames_cached} cached)")

        # reference calculators.py:218-221 (quirk Q2: `sampling`, not dx; torch default float32)
        kxs, kys = self._k_axes()
        time_array = np.arange(self.n_frames) * self.trajectory.timestep
        layer_array = np.array([0]) if self._layers_arg is None else np.asarray(self._layers, dtype=np.int64)   # (layers: slice indices)

        data, resident = self._collect()
        self.wavefunction_data = data
        wf = WFData(probe_positions=self.probe_positions, time=time_array, kxs=_as_tensor(kxs), kys=_as_tensor(kys),
                    layer=layer_array, wavefunction_data=data, probe=self.base_probe)
        # private riders: let TACAWData transform the device-resident copy without a host round trip
        self._tag_crop(wf)
        wf._engine = eng
        wf._resident = resident
        wf._output = self._output
        if self._world > 1 and self._gather == "none":
            wf._frame_shard = (self.n_frames, len(frames))      # lets TACAWData do the all-to-all itself
        return wf

    def _k_axes(self):
        """kxs, kys of the stored spectra: reference calculators.py:218-219 (quirk Q2), cropped to the k-window (centred on
        the DC pixel, index n//2 after the shift) and averaged over every detector bin.  Of a cropped PRISM run: the axes of the
        cropped grid, h / (n_c d) -- the full axes at prism.crop_index"""
        nx, ny = self._result_grid()
        kxs = np.fft.fftshift(np.fft.fftfreq(nx, self.sampling)).astype(np.float32)
        kys = np.fft.fftshift(np.fft.fftfreq(ny, self.sampling)).astype(np.float32)
        if self._k_window is not None:
            wx, wy = self._k_window
            x0, y0 = nx // 2 - wx // 2, ny // 2 - wy // 2
            kxs, kys = kxs[x0:x0 + wx], kys[y0:y0 + wy]
        if self._k_bin is not None:
            kxs = kxs.reshape(-1, self._k_bin[0]).mean(axis=1).astype(np.float32)
            kys = kys.reshape(-1, self._k_bin[1]).mean(axis=1).astype(np.float32)
        return kxs, kys

    def run_streaming_tacaw(self, freq_window=None, bins=None):
        """Streaming TACAW (needs stream_tile): all frames are propagated through a ring of `stream_tile` frame slots and
        folded, tile by tile, into the time->frequency transform of the selected bins.

        freq_window = (lo, hi): keep the bins of TACAWData.frequencies (fftshifted, reference tacaw_data.py:84-85) with
        lo <= f <= hi;  bins = explicit indices into that fftshifted axis;  neither: all T bins.
        Returns a TACAWData whose `frequencies` / `intensity` hold the selected bins only ((P,F,wx,wy), device-resident
        for the reductions), plus `total_diffraction` (P,wx,wy): the sum over ALL T bins (Parseval), i.e. what
        TACAWData.diffraction() of the full transform returns, without the transform being stored."""
        from .tacaw_data import TACAWData
        if getattr(self, "_coherence", None) is not None:
            raise NotImplementedError("coherence: run_streaming_tacaw() is not built")
        if self._engine is None:
            raise RuntimeError("call setup() before run_streaming_tacaw()")
        if self._stream_tile is None:
            raise RuntimeError("run_streaming_tacaw() needs MultisliceCalculator(stream_tile=Tt)")
        if self._layers is not None and len(self._layers) > 1:
            raise ValueError("run_streaming_tacaw() keeps the exit wave only: no layers")
        eng, T = self._engine, self.n_frames
        if T < 2:
            raise ValueError("TACAW needs at least 2 frames")
        time_array = np.arange(T) * self.trajectory.timestep
        freqs = np.fft.fftshift(np.fft.fftfreq(T, d=time_array[1] - time_array[0]))
        if bins is not None:
            sel = np.asarray(bins, dtype=np.int64).reshape(-1)
            if sel.size == 0 or sel.min() < 0 or sel.max() >= T:
                raise ValueError(f"bins must be indices into the {T} fftshifted frequencies")
        elif freq_window is not None:
            sel = np.nonzero((freqs >= freq_window[0]) & (freqs <= freq_window[1]))[0]
            if sel.size == 0:
                raise ValueError(f"no frequency bin inside {freq_window}")
        else:
            sel = np.arange(T)
        unshifted = (sel + (T + 1) // 2) % T              # fftshifted index s holds FFT bin (s + ceil(T/2)) mod T
        t0 = time.time()
        eng.tacaw_stream_begin(T, unshifted)
        ring, B = eng.n_frames, eng.frame_batch
        # This rank's MD frames (all of them in a single-process run): propagated through the ring tile by tile and folded with
        # their GLOBAL time indices.  The first frame of the run is the reference pattern every rank subtracts before folding
        # (msl_tacaw_stream_set_reference): rank 0 takes it from its first tile and broadcasts it (P x stored pixels, once).
        frames = self._frames
        have_ref = False
        for tile0 in range(0, max(len(frames), 1), ring):
            tile = frames[tile0:tile0 + ring]
            for s0 in range(0, len(tile), B):
                chunk = tile[s0:s0 + B]
                self._build_and_propagate(chunk[0], len(chunk), s0)
            if not have_ref:
                self._stream_reference(eng)
                have_ref = True
            if tile:
                eng.tacaw_stream_push(0, len(tile), tile[0])
        kxs, kys = self._k_axes()
        tac = TACAWData.__new__(TACAWData)
        tac.__dict__.update(dict(probe_positions=self.probe_positions, time=time_array, kxs=_as_tensor(kxs), kys=_as_tensor(kys),
                                 layer=np.array([0]), wavefunction_data=None, probe=self.base_probe,
                                 frequencies=freqs[sel], frequency_bins=sel, _engine=eng, _output=self._output))
        if self._world > 1:
            self._finish_stream_sharded(eng, tac)
            self.elapsed = time.time() - t0
            return tac
        total = eng.tacaw_stream_finish(True)
        self.elapsed = time.time() - t0
        tac.total_diffraction = total
        tac._intensity_src = (eng, None)
        if self._output == "device":
            tac.intensity = torch.as_tensor(eng.result_view(_native.BUF_INTENSITY, "<f4"), device=f"cuda:{eng.device}")
        else:
            tac.intensity = _as_tensor(eng.intensity().astype(np.float64))
        return tac

    def _stream_reference(self, eng):
        """the run's first frame (frame slot 0 of rank 0's first tile) becomes the reference pattern of every rank's fold"""
        if self._world == 1:
            eng.tacaw_stream_set_reference(slot=0)
            return
        dev = torch.device("cuda", eng.device)
        P, K = eng.n_probes, eng.wx * eng.wy
        if self._rank == 0:
            eng.tacaw_stream_set_reference(slot=0)
            eng.synchronize()
            ref = torch.as_tensor(_native.DeviceArray(eng.device_ptr(_native.BUF_STREAM_REF), (P, K), "<c8", owner=eng), device=dev)
            distributed.broadcast_from(ref, src=0)
        else:
            ref = torch.empty((P, K), dtype=torch.complex64, device=dev)
            distributed.broadcast_from(ref, src=0)
            torch.cuda.synchronize(dev)
            eng.tacaw_stream_set_reference(ref_ptr=ref.data_ptr())
            eng.synchronize()                     # the copy out of `ref` is done before the tensor goes away

    def _finish_stream_sharded(self, eng, tac):
        """Frame-sharded streaming TACAW: sum the ranks' partial sums (reduce-scatter over probes, distributed.reduce_probes),
        finish this rank's probes, gather the intensities (distributed.gather_probes).  tacaw_data.py:89-104 on an array no
        rank ever holds."""
        dev = torch.device("cuda", eng.device)
        P, F, K = eng.n_probes, len(tac.frequency_bins), eng.wx * eng.wy
        eng.synchronize()

        def view(what, shape, typestr):
            return torch.as_tensor(_native.DeviceArray(eng.device_ptr(what), shape, typestr, owner=eng), device=dev)
        p0, p1 = distributed.reduce_probes(view(_native.BUF_STREAM_ACC, (P, F, K), "<c8"), P)
        distributed.reduce_probes(view(_native.BUF_STREAM_S1, (P, K, 2), "<f8"), P)
        distributed.reduce_probes(view(_native.BUF_STREAM_S2, (P, K), "<f8"), P)
        torch.cuda.synchronize(dev)
        mine = torch.empty((p1 - p0, F, eng.wx, eng.wy), dtype=torch.float32, device=dev)
        total = eng.tacaw_stream_finish_range(p0, p1 - p0, mine.data_ptr(), True)       # (an empty shard still closes the stream)
        tot = torch.from_numpy(total).to(dev)
        tac.probe_range = (p0, p1)
        if self._gather == "none":
            # this rank keeps ITS probes only: the TACAWData's probe list is the shard's (its methods index probes by
            # len(probe_positions)); probe_range holds the shard's place in the run's probe list
            full, tot_full = mine, tot
            tac.probe_positions = list(tac.probe_positions)[p0:p1]
        else:
            dst = None if self._gather == "all" else 0
            full = distributed.gather_probes(mine, P, dst=dst)
            tot_full = distributed.gather_probes(tot, P, dst=dst)
        if full is None:
            tac.intensity, tac.total_diffraction = None, None
            return
        tac._intensity_src = (eng, full)
        tac.total_diffraction = tot_full.cpu().numpy()
        tac.intensity = full if self._output == "device" else full.to(torch.float64).cpu()

    # ------------------------------------------------------------------------------------------
    def _collect(self):
        """Pack the device-resident (P,T_local,nx,ny) into the reference's (P,T,nx,ny,1) array."""
        eng = self._engine
        P, nx, ny = self.n_probes, eng.wx, eng.wy          # stored spectrum shape (the k-window, or the grid)
        T_local = len(self._frames)
        if eng.n_layers > 1:
            # (layers: single-process runs only) the (L, P, T, wx, wy) device result -> the reference's (P, T, wx, wy, L)
            if self._output == "device":
                view = torch.as_tensor(eng.layers_view(), device=f"cuda:{eng.device}")
                return view.permute(1, 2, 3, 4, 0)[:, :T_local], T_local == eng.n_frames
            if self._dtype == "complex128":
                return _as_tensor(eng.layers_c128(T_local)), T_local == eng.n_frames
            local = eng.layers_c64()[:, :, :T_local]
            return _as_tensor(np.ascontiguousarray(np.moveaxis(local, 0, -1))), T_local == eng.n_frames
        if self._world == 1 or self._gather == "none":
            if self._output == "device":
                # (the images sit at the library's line-aligned pixel pitch: a strided view when nx*ny is not a multiple of 32)
                view = torch.as_tensor(eng.result_view(_native.BUF_WAVEFUNCTION, "<c8"), device=f"cuda:{eng.device}")
                return view[:, :T_local].unsqueeze(-1), T_local == eng.n_frames
            if self._dtype == "complex128":
                # the reference's dtype: widened on the device and copied out as complex128 (msl_download_wavefunction_c128) --
                # the single-threaded numpy astype on the host took twice the whole multislice run of the default single-probe
                # case (501 x 491 x 100 frames: run() 0.171 s, of which 0.051 s on the GPU)
                return _as_tensor(eng.wavefunction_c128(T_local)[..., None]), T_local == eng.n_frames
            local = eng.wavefunction()[:, :T_local]
            return _as_tensor(np.ascontiguousarray(local[..., None])), T_local == eng.n_frames
        # multi-process: one gather of the frame shards (no collective during the frames)
        local = torch.as_tensor(eng.result_view(_native.BUF_WAVEFUNCTION, "<c8"), device=f"cuda:{eng.device}")[:, :T_local]
        full = distributed.gather_frames(local, self.n_frames, dst=None if self._gather == "all" else 0)
        if full is None:
            return None, False
        if self._output == "device":
            return full.unsqueeze(-1), False
        full = _widen_to_host(full) if self._dtype == "complex128" else full.cpu()
        return full.unsqueeze(-1), False

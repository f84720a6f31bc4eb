"""Frame-averaged diffraction patterns per probe position (CBED / 4D-STEM), streamed over probe batches
(MultisliceCalculator(diffraction=Diffraction(bin=...)).run_diffraction()).

The HIP pass msl_diffract (pyslice_amd/csrc/diffract.h) turns the exit spectra of a probe batch into |Psi|^2 summed over the
frames of the batch and over every bx x by block of stored pixels -- the intensity a pixelated detector records, not the
coherent block sum of k_bin -- as soon as the slice loop has written them.  A scan therefore needs no (P, T, nx, ny) array:
DiffractionData holds the (P, mx, my) frozen-phonon mean only, and everything below is NumPy on that small result.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, Optional, Tuple

import numpy as np

from .stem_data import Detector, STEMData, scan_axes, scan_image


class Diffraction:
    """The request: bin=(bx, by) stored pixels per detector pixel along kx and ky (both must divide the stored spectrum);
    split=True also asks for the elastic part |<Psi>|^2 of every pattern (DiffractionData.elastic / .tds), which costs one
    potential build per probe batch and frame instead of one per frame (MultisliceCalculator.run_diffraction).
    dose=dose.Dose(...) asks for Poisson-counted patterns at that dose, drawn on the device (DiffractionData.counts); it takes the
    loop order of the split, at the same price, and is not built together with it.
    camera=camera.Camera(...), with a dose, turns the counts into the uint16 frames a camera writes, on the device
    (DiffractionData.frames)."""

    def __init__(self, bin=(1, 1), split=False, dose=None, camera=None):
        try:
            ok = len(bin) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and int(v) >= 1 for v in bin)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"Diffraction: bin must be two positive integers (bx, by), got {bin!r}")
        if not isinstance(split, (bool, np.bool_)):
            raise ValueError(f"Diffraction: split must be True or False, got {split!r}")
        if dose is not None:
            from .dose import Dose
            if not isinstance(dose, Dose):
                raise ValueError(f"Diffraction: dose must be a Dose object, got {dose!r}")
            if split:
                raise NotImplementedError("dose: split=True is not built")
        if camera is not None:
            from .camera import Camera
            if not isinstance(camera, Camera):
                raise ValueError(f"Diffraction: camera must be a Camera object, got {camera!r}")
            if dose is None:
                raise ValueError("Diffraction: a camera records the counts of a dose: give dose=Dose(...) as well")
        self.bin = (int(bin[0]), int(bin[1]))
        self.split = bool(split)
        self.dose = dose
        self.camera = camera

    def __repr__(self):
        return (f"Diffraction(bin={self.bin}" + (", split=True" if self.split else "")
                + (f", dose={self.dose!r}" if self.dose is not None else "")
                + (f", camera={self.camera!r}" if self.camera is not None else "") + ")")


def bin_centres(axis, b):
    """bin-centre axis: the mean of every b consecutive values of a stored k axis, float32 (as MultisliceCalculator's k_bin axes)"""
    a = np.asarray(axis.detach().cpu().numpy() if hasattr(axis, "detach") else axis, dtype=np.float32)
    if a.size % b:
        raise ValueError(f"an axis of {a.size} values is not a multiple of the bin {b}")
    return a.reshape(-1, b).mean(axis=1).astype(np.float32)


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@dataclass
class DiffractionData:
    """Result of MultisliceCalculator.run_diffraction(): intensity (P, mx, my) float64 -- the mean over the n_frames MD frames of
    |Psi|^2 in detector pixel (ix, iy) at probe p --, the bin-centre axes kxs / kys (float32), the bin, the run's
    probe_positions / probe / wavelength, the scan axes xs / ys, and `stem`: the STEMData of the same pass when the run had detectors.
    With Diffraction(split=True), `elastic` (P, mx, my) float64 is |<Psi>|^2 -- the coherent mean over the frames, squared, then
    summed over the pixels of the bin (a bin adds intensities) --, `tds` the thermal diffuse rest, and part() gives either as a
    DiffractionData of its own; `elastic` is None otherwise.
    With MultisliceCalculator(thickness=...) intensity is (P, mx, my, L): `layer` holds the slice indices of the L thickness entries,
    `thickness` the depth in Angstrom at the exit side of each slice, at(i) is the ordinary DiffractionData of entry i (its stem
    too), and pacbed / virtual / image / pattern take layer=-1, the exit wave.  With Thickness(patterns="pacbed") only the
    position-averaged pattern was kept: intensity is (mx, my, L) -- (mx, my) after at(i) -- which pacbed() returns and the
    per-position methods refuse.
    With Diffraction(dose=Dose(...)) `counts` (P, mx, my) uint32 holds the electrons every detector pixel recorded at
    `electrons_per_probe` incident electrons per position (dose.py is the definition of the draw; `dose` the request, `incident` the
    spectrum-intensity sum of the incident probe, so that the expected count of a pixel is intensity * electrons_per_probe /
    incident); `intensity` is the noise-free mean only with Dose(keep_intensity=True), None otherwise.  pacbed / virtual / image /
    pattern then work on the counts, in electrons as float64, and take part="counts" | "intensity" when both are there.
    With Diffraction(dose=..., camera=Camera(...)) `frames` (P, mx, my) uint16 holds what the camera wrote (camera.py is the
    definition; `camera` the request); `counts` is there only with Camera(keep_counts=True).  part="frames" reads the frames back in
    electrons, (frames - offset) / gain as float64, and is the default when frames are all there is.  datacube() is the
    (sx, sy, mx, my) array of a raster scan."""
    intensity: Optional[np.ndarray]
    kxs: Any
    kys: Any
    bin: Tuple[int, int]
    n_frames: int
    probe_positions: Any
    probe: Any
    stem: Optional[STEMData] = None
    wavelength: Optional[float] = None      # Angstrom; None: the probe's
    xs: np.ndarray = None
    ys: np.ndarray = None
    elastic: Optional[np.ndarray] = None
    layer: Optional[np.ndarray] = None
    thickness: Optional[np.ndarray] = None
    patterns: str = "position"
    tilts: Optional[list] = None            # the tilt.Tilt of every run of a precession average (tilt order); None otherwise
    counts: Optional[np.ndarray] = None
    dose: Any = None
    electrons_per_probe: Optional[float] = None
    incident: Optional[float] = None
    frames: Optional[np.ndarray] = None
    camera: Any = None
    coherence: Any = None                   # the coherence.Coherence of the run (None: a coherent probe)

    def __post_init__(self):
        if self.patterns not in ("position", "pacbed"):
            raise ValueError(f"patterns must be 'position' or 'pacbed', got {self.patterns!r}")
        if self.intensity is None and self.counts is None and self.frames is None:
            raise ValueError("DiffractionData needs intensity or counts")
        if self.frames is not None:
            if self.layer is not None or self.patterns != "position" or np.ndim(self.frames) != 3:
                raise ValueError("frames are per-position patterns (P, mx, my) without a thickness axis")
            if self.camera is None:
                raise ValueError("frames need the camera that wrote them")
            for name, other in (("counts", self.counts), ("intensity", self.intensity)):
                if other is not None and np.shape(other) != np.shape(self.frames):
                    raise ValueError(f"frames have shape {np.shape(self.frames)}, {name} {np.shape(other)}")
        if self.counts is not None:
            if self.layer is not None or self.patterns != "position" or np.ndim(self.counts) != 3:
                raise ValueError("counts are per-position patterns (P, mx, my) without a thickness axis")
            if self.intensity is not None and np.shape(self.intensity) != np.shape(self.counts):
                raise ValueError(f"counts have shape {np.shape(self.counts)}, intensity {np.shape(self.intensity)}")
        want = (3 if self.patterns == "position" else 2) + (self.layer is not None)
        if (self.layer is not None or self.patterns == "pacbed") and (
                np.ndim(self.intensity) != want or (self.layer is not None and np.shape(self.intensity)[-1] != len(self.layer))):
            raise ValueError(f"intensity of shape {np.shape(self.intensity)} for patterns={self.patterns!r}"
                             + ("" if self.layer is None else f" and {len(self.layer)} thickness entries"))
        if self.elastic is not None and np.shape(self.elastic) != np.shape(self.intensity):
            raise ValueError(f"elastic has shape {np.shape(self.elastic)}, intensity {np.shape(self.intensity)}")
        if self.wavelength is None and self.probe is not None:
            self.wavelength = float(self.probe.wavelength)
        if self.xs is None or self.ys is None:
            self.xs, self.ys = scan_axes(self.probe_positions)

    def at(self, i: int) -> "DiffractionData":
        """the un-layered DiffractionData of thickness entry i (negative from the end: -1 is the exit wave)"""
        if self.layer is None:
            raise ValueError("this DiffractionData has no thickness axis: run with MultisliceCalculator(thickness=...)")
        from .thickness import entry
        j = entry(self.layer, i)
        return replace(self, intensity=self.intensity[..., j], layer=None, thickness=None,
                       stem=None if self.stem is None else self.stem.at(j))

    def _data(self, part=None):
        """the array the reductions read: part=None is the intensity as ever, the counts (as float64 electrons) when there is
        no intensity, and the frames (read back in electrons) when they are all there is; "counts" / "intensity" / "frames" name one"""
        if part not in (None, "counts", "intensity", "frames"):
            raise ValueError(f"part must be 'counts' or 'intensity', got {part!r}" if self.frames is None else
                             f"part must be 'counts', 'intensity' or 'frames', got {part!r}")
        if part is None:
            part = "intensity" if self.intensity is not None else "counts" if self.counts is not None or self.frames is None else "frames"
        if part == "frames":
            if self.frames is None:
                raise ValueError("this DiffractionData has no frames: run with Diffraction(dose=Dose(...), camera=Camera(...))")
            from .camera import electrons
            return electrons(self.frames, self.camera)
        arr = self.counts if part == "counts" else self.intensity
        if arr is None:
            raise ValueError("this DiffractionData has no counts: run with Diffraction(dose=Dose(...))" if part == "counts" else
                             "this DiffractionData has no intensity: run with Dose(keep_intensity=True)")
        return arr.astype(np.float64) if part == "counts" else arr

    def _per_position(self, what):
        if self.patterns != "position":
            raise ValueError(f"{what}: this DiffractionData holds the position-averaged pattern only (Thickness(patterns='pacbed'))")

    @property
    def tds(self) -> np.ndarray:
        """(P, mx, my): the thermal diffuse part <|Psi|^2> - |<Psi>|^2, the energy-integrated TACAW intensity divided by T^2.
        Not clamped: where nothing is diffuse (one frame, no displacements) the float32 rounding of the pattern pass, about
        1e-7 of the total per addend, can leave it that far below zero."""
        if self.elastic is None:
            raise ValueError("this DiffractionData has no elastic part: run with Diffraction(split=True)")
        return self.intensity - self.elastic

    def part(self, name: str) -> "DiffractionData":
        """the DiffractionData whose intensity is the "total", "elastic" or "tds" part (axes, probes and stem shared; its own
        `elastic` is None), so that pacbed(), virtual(), image() and pattern() work on each part"""
        if name not in ("total", "elastic", "tds"):
            raise ValueError(f"part: expected 'total', 'elastic' or 'tds', got {name!r}")
        if self.elastic is None:
            raise ValueError("this DiffractionData has no elastic part: run with Diffraction(split=True)")
        arr = {"total": self.intensity, "elastic": self.elastic, "tds": None}[name]
        return replace(self, intensity=self.tds if arr is None else arr, elastic=None)

    def pacbed(self, layer=-1, part=None) -> np.ndarray:
        """(mx, my): position-averaged pattern, the mean over the probes; of thickness entry `layer` when there is a thickness axis"""
        if self.layer is not None:
            return self.at(layer).pacbed(part=part)
        data = self._data(part)
        return data if self.patterns == "pacbed" else data.mean(axis=0)

    def member(self, detector: Detector) -> np.ndarray:
        """(mx, my) bool: the detector pixels whose CENTRE lies in `detector` (its member() on the bin-centre axes)"""
        if not isinstance(detector, Detector):
            raise ValueError(f"expected a Detector, got {detector!r}")
        if detector.signal != "intensity":
            raise ValueError(f"detector {detector.name!r}: patterns hold |Psi|^2 only, signal {detector.signal!r} cannot be formed from them")
        if self.wavelength is None:
            raise ValueError("DiffractionData has neither a probe nor a wavelength: detector angles cannot be turned into k")
        return detector.member(_np(self.kxs), _np(self.kys), self.wavelength)

    def virtual(self, detector: Detector, layer=-1, part=None) -> np.ndarray:
        """(P,): the virtual detector chosen after the run -- sum of the detector pixels inside `detector`"""
        if self.layer is not None:
            return self.at(layer).virtual(detector, part=part)
        self._per_position("virtual()")
        m = self.member(detector)
        return (self._data(part) * m[None].astype(np.float64)).sum(axis=(-2, -1))

    def image(self, detector: Detector, layer=-1, part=None) -> np.ndarray:
        """(len(xs), len(ys)) scan image of virtual(detector): every scan point takes its nearest probe's value (STEMData.image)"""
        return scan_image(self.virtual(detector, layer, part), self.probe_positions, self.xs, self.ys)

    def pattern(self, x: float, y: float, layer=-1, part=None) -> np.ndarray:
        """(mx, my): the pattern of the probe nearest to (x, y)"""
        if self.layer is not None:
            return self.at(layer).pattern(x, y, part=part)
        self._per_position("pattern()")
        pp = np.asarray(self.probe_positions, dtype=np.float64).reshape(-1, 2)
        return self._data(part)[int(np.argmin(((pp - np.array([x, y])[None, :]) ** 2).sum(axis=1)))]

    def datacube(self, part=None) -> np.ndarray:
        """(len(xs), len(ys), mx, my): the patterns of a scan on a regular raster, ordered by scan position -- the 4D array that
        4D-STEM packages load.  part=None: the array as it was recorded (frames uint16, else counts uint32, else the intensity);
        "frames" / "counts" / "intensity" name one, as recorded too (no conversion to electrons).  ValueError unless every raster
        point (xs[i], ys[j]) holds exactly one probe."""
        self._per_position("datacube()")
        if self.layer is not None:
            raise ValueError("datacube(): take one thickness entry first (at(i))")
        if part not in (None, "counts", "intensity", "frames"):
            raise ValueError(f"part must be 'counts', 'intensity' or 'frames', got {part!r}")
        if part is None:
            part = "frames" if self.frames is not None else "counts" if self.counts is not None else "intensity"
        arr = {"frames": self.frames, "counts": self.counts, "intensity": self.intensity}[part]
        if arr is None:
            raise ValueError(f"this DiffractionData has no {part}")
        pp = np.asarray(self.probe_positions, dtype=np.float64).reshape(-1, 2)
        sx, sy = len(self.xs), len(self.ys)
        if sx * sy != len(pp) or len({(x, y) for x, y in pp}) != len(pp):
            raise ValueError(f"datacube(): {len(pp)} probe positions are not a full {sx} x {sy} raster of their coordinates")
        index = scan_image(np.arange(len(pp), dtype=np.float64), pp, self.xs, self.ys).astype(np.int64)
        return arr[index.reshape(-1)].reshape((sx, sy) + arr.shape[1:])

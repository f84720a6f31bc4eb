"""STEM detector images streamed over probe batches (MultisliceCalculator(detectors=[...]).run_detectors()).

A Detector is a region of the stored exit-wave spectrum (an annulus, optionally an azimuthal segment of it) and a signal.
The HIP pass msl_detect (pyslice_amd/csrc/detect.h) reduces every exit spectrum to its detector values on the device as soon
as the slice loop has written it, so a scan needs no (P, T, nx, ny) array: STEMData holds the (P, T, D) signals only.
`Detector("adf", inner=collection_angle, signal="amplitude")` is exactly HAADFData.calculateADF's mask and sum
(reference haadf_data.py:44-68).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from ._native import DET_SIGNALS

MAX_DETECTORS = 16


@dataclass(frozen=True)
class Detector:
    """name; inner / outer collection angles in mrad (outer=None: no outer edge); azimuth=(phi0, phi1) in degrees with
    phi = atan2(ky, kx) in [0, 360), the segment phi0 <= phi < phi1 (wrapping through 0 when phi0 > phi1); signal one of
    "intensity" (|Psi|^2), "amplitude" (|Psi|, the HAADFData convention), "com_x" (kx |Psi|^2), "com_y" (ky |Psi|^2)."""
    name: str
    inner: float = 0.0
    outer: Optional[float] = None
    azimuth: Optional[Tuple[float, float]] = None
    signal: str = "intensity"

    def __post_init__(self):
        if not isinstance(self.name, str) or not self.name:
            raise ValueError("a detector needs a non-empty name")
        if not np.isfinite(self.inner) or self.inner < 0:
            raise ValueError(f"detector {self.name!r}: inner angle must be >= 0 mrad, got {self.inner}")
        if self.outer is not None and (not np.isfinite(self.outer) or self.outer < 0):
            raise ValueError(f"detector {self.name!r}: outer angle must be >= 0 mrad, got {self.outer}")
        if self.outer is not None and self.outer <= self.inner:
            raise ValueError(f"detector {self.name!r}: outer angle {self.outer} must exceed the inner angle {self.inner}")
        if self.signal not in DET_SIGNALS:
            raise ValueError(f"detector {self.name!r}: unknown signal {self.signal!r} (one of {sorted(DET_SIGNALS)})")
        if self.azimuth is not None:
            a = tuple(float(v) for v in self.azimuth)
            if len(a) != 2 or not all(0.0 <= v <= 360.0 for v in a) or a[0] == a[1]:
                raise ValueError(f"detector {self.name!r}: azimuth must be two different angles in [0, 360] degrees, got {self.azimuth}")
            object.__setattr__(self, "azimuth", a)

    def member(self, kxs, kys, wavelength) -> np.ndarray:
        """(len(kxs), len(kys)) bool: the stored pixels inside this detector.  kxs / kys are WFData's float32 axes, widened to
        float64; q and the edge radius are formed as HAADFData.calculateADF forms them (haadf_data.py:46-49)."""
        kx = np.asarray(kxs, dtype=np.float32).astype(np.float64)
        ky = np.asarray(kys, dtype=np.float32).astype(np.float64)
        q = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
        sel = np.ones(q.shape, dtype=bool)
        if self.inner != 0:
            sel &= q > (self.inner * 1e-3) / wavelength
        if self.outer is not None:
            sel &= q <= (self.outer * 1e-3) / wavelength
        if self.azimuth is not None:
            phi = np.degrees(np.arctan2(ky[None, :], kx[:, None])) % 360.0
            phi = np.where(phi >= 360.0, phi - 360.0, phi)
            p0, p1 = self.azimuth
            sel &= ((phi >= p0) & (phi < p1)) if p0 < p1 else ((phi >= p0) | (phi < p1))
        return sel


def check_detectors(detectors: Sequence[Detector]) -> List[Detector]:
    """the `detectors` argument of MultisliceCalculator -> a list of Detector (ValueError before any device work)"""
    dets = list(detectors)
    if not dets:
        raise ValueError("detectors: give at least one Detector")
    if len(dets) > MAX_DETECTORS:
        raise ValueError(f"detectors: at most {MAX_DETECTORS} detectors, got {len(dets)}")
    for d in dets:
        if not isinstance(d, Detector):
            raise ValueError(f"detectors: expected Detector objects, got {d!r}")
    names = [d.name for d in dets]
    if len(set(names)) != len(names):
        raise ValueError(f"detectors: duplicate names in {names}")
    return dets


def detector_bitmask(detectors: Sequence[Detector], kxs, kys, wavelength) -> np.ndarray:
    """(wx, wy) uint16: bit d set where pixel (i, j) lies in detector d (the msl_set_detectors membership)"""
    out = np.zeros((len(kxs), len(kys)), dtype=np.uint16)
    for d, det in enumerate(detectors):
        out |= det.member(kxs, kys, wavelength).astype(np.uint16) << np.uint16(d)
    return out


def scan_axes(probe_positions) -> Tuple[np.ndarray, np.ndarray]:
    """xs, ys of a scan: the sorted unique probe coordinates (HAADFData.calculateADF, haadf_data.py:44-45)"""
    pp = np.asarray(probe_positions, dtype=np.float64).reshape(-1, 2)
    return np.asarray(sorted(set(pp[:, 0]))), np.asarray(sorted(set(pp[:, 1])))


def scan_image(per_probe, probe_positions, xs, ys) -> np.ndarray:
    """(len(xs), len(ys)): every scan point takes the value of its nearest probe (HAADFData's assignment, haadf_data.py:81-86)"""
    pp = np.asarray(probe_positions, dtype=np.float64).reshape(-1, 2)
    v = np.asarray(per_probe)
    img = np.zeros((len(xs), len(ys)))
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            p = int(np.argmin(np.sqrt(((pp - np.array([x, y])[None, :]) ** 2).sum(axis=1))))
            img[i, j] = v[p]
    return img


@dataclass
class STEMData:
    """Result of MultisliceCalculator.run_detectors(): signals (P, T, D) float64 -- detector d of frame t at probe p --, the
    detectors, the run's probe_positions / time / kxs / kys / probe, and the scan axes xs, ys.
    With MultisliceCalculator(thickness=...) signals is (P, T, D, L): `layer` holds the slice indices of the L thickness entries,
    `thickness` the depth in Angstrom at the exit side of each slice, at(i) is the ordinary STEMData of entry i, and image() takes
    layer=-1, the exit wave.
    With MultisliceCalculator(tds=True) signals is the elastic part and tds_per_slice (P, T, D, nz) the thermal diffuse signal that
    every slice generates on every detector (tds.py, times nx ny: the units of the unnormalised spectra the signals sum): `tds` is its sum over the slices -- with a thickness axis its cumulative sum at
    the entries, (P, T, D, L) --, `total` = signals + tds, and image() takes part="total" | "elastic" | "tds"."""
    signals: np.ndarray
    detectors: List[Detector]
    probe_positions: Any
    time: np.ndarray
    kxs: Any
    kys: Any
    probe: Any
    xs: np.ndarray = None
    ys: np.ndarray = None
    layer: Optional[np.ndarray] = None
    thickness: Optional[np.ndarray] = None
    tilts: Optional[list] = None            # the tilt.Tilt of every run of a precession average (tilt order); None otherwise
    tds_per_slice: Optional[np.ndarray] = None
    coherence: Any = None                   # the coherence.Coherence of the run (None: a coherent probe)

    def source_blurred(self, sigma, periodic=True) -> "STEMData":
        """this result with the signals convolved over the scan with a Gaussian source of rms width sigma (Angstrom) per axis
        (coherence.blur_scan): the cheap route to a finite source size.  The probe positions must form a full regular raster
        (ValueError otherwise); periodic=True when the raster covers a periodic cell."""
        from .coherence import blur_positions
        return replace(self, signals=blur_positions(self.signals, self.probe_positions, sigma, periodic),
                       tds_per_slice=None if self.tds_per_slice is None else blur_positions(self.tds_per_slice, self.probe_positions,
                                                                                           sigma, periodic))

    def __post_init__(self):
        if self.xs is None or self.ys is None:
            self.xs, self.ys = scan_axes(self.probe_positions)
        if self.layer is not None and (np.ndim(self.signals) != 4 or np.shape(self.signals)[-1] != len(self.layer)):
            raise ValueError(f"signals of shape {np.shape(self.signals)} for {len(self.layer)} thickness entries")

    def at(self, i: int) -> "STEMData":
        """the un-layered STEMData of thickness entry i (negative from the end: -1 is the exit wave)"""
        if self.layer is None:
            raise ValueError("this STEMData has no thickness axis: run with MultisliceCalculator(thickness=...)")
        from .thickness import entry
        tps = self.tds_per_slice
        if tps is not None:                 # the slices up to the entry: what has been generated by then
            tps = tps[..., :int(self.layer[entry(self.layer, i)]) + 1]
        return replace(self, signals=self.signals[..., entry(self.layer, i)], layer=None, thickness=None, tds_per_slice=tps)

    @property
    def tds(self) -> np.ndarray:
        """(P, T, D), the TDS on every detector summed over the slices; (P, T, D, L) with a thickness axis: the cumulative sum at
        the slice of every entry"""
        if self.tds_per_slice is None:
            raise ValueError("this STEMData has no TDS signal: run with MultisliceCalculator(tds=True)")
        if self.layer is None:
            return self.tds_per_slice.sum(axis=-1)
        return np.cumsum(self.tds_per_slice, axis=-1)[..., np.asarray(self.layer, dtype=np.int64)]

    @property
    def total(self) -> np.ndarray:
        """signals + tds: the elastic part and the thermal diffuse part of every detector"""
        return self.signals + self.tds

    def poisson(self, dose, seed=None) -> np.ndarray:
        """(P, D) uint32 -- (P, D, L) with a thickness axis: the electrons every detector counts at `dose` (electrons per probe
        position, or a dose.Dose), drawn on the host by dose.poisson_counts from the frame mean of the signals per incident electron;
        probe p keyed by its index, the pixel index the row-major index of the rest.  seed=None: the Dose's seed (0 for a number).
        Intensity detectors only: an amplitude or a centre of mass is no count."""
        from .dose import Dose, poisson_signals, probe_incident
        bad = [d.name for d in self.detectors if d.signal != "intensity"]
        if bad:
            raise ValueError(f"poisson(): detectors {bad} do not have the intensity signal; counts are defined for intensities only")
        n_e = dose.electrons(self.probe_positions) if isinstance(dose, Dose) else dose
        if seed is None:
            seed = dose.seed if isinstance(dose, Dose) else 0
        return poisson_signals(np.asarray(self.signals, dtype=np.float64).mean(axis=1), n_e, probe_incident(self.probe), seed)

    def index(self, name: str) -> int:
        for d, det in enumerate(self.detectors):
            if det.name == name:
                return d
        raise KeyError(f"no detector named {name!r} (have {[d.name for d in self.detectors]})")

    def image(self, name: str, frames=None, layer=-1, part=None) -> np.ndarray:
        """(len(xs), len(ys)) image of detector `name`: mean over the frames (all, or an index / slice / list of frame
        indices) on the scan grid, every scan point taking its nearest probe's value as HAADFData does; of thickness entry
        `layer` when there is a thickness axis.  part: "elastic" (signals), "tds" or "total" of a run with tds=True; None is "total"
        there and the signals otherwise."""
        if part not in (None, "total", "elastic", "tds"):
            raise ValueError(f"part must be 'total', 'elastic' or 'tds', got {part!r}")
        if part in ("total", "tds") and self.tds_per_slice is None:
            raise ValueError(f"part={part!r} needs a run with MultisliceCalculator(tds=True)")
        if self.layer is not None:
            return self.at(layer).image(name, frames, part=part)
        if part is None:
            part = "elastic" if self.tds_per_slice is None else "total"
        s = {"elastic": lambda: self.signals, "tds": lambda: self.tds, "total": lambda: self.total}[part]()[:, :, self.index(name)]
        if frames is not None:
            s = s[:, frames]
            if s.ndim == 1:
                s = s[:, None]
        return scan_image(s.mean(axis=1), self.probe_positions, self.xs, self.ys)

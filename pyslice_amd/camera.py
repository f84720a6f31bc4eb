"""Detector response: what a camera writes for the electrons that landed on it -- point spread, gain, dark offset, readout noise and
a clipped integer per pixel.

dose.py returns the electrons that landed on every detector pixel: an ideal counting detector.  A camera spreads each electron over
neighbouring pixels (its point-spread function; the modulus of its transform is the MTF), multiplies by a gain, sits on a dark
offset, adds readout noise and writes a clipped unsigned integer of `bits` bits.  This file is the definition of that response, in
NumPy, float64; the device computes the same frames itself (csrc/camera.h: camera_frames_kernel behind msl_camera_frames and
msl_dose_frames), where the counts already are, so a 4D-STEM scan downloads 2 bytes per detector pixel.

For pixel (ix, iy) of the (mx, my) pattern of probe p (its index in the scan, as in dose.py), with c the counts as float64, zero
outside the pattern, and r the radius of the (2r+1, 2r+1) table psf:

    s = 0.0;  for a = -r .. r:  for b = -r .. r:   s = s + psf[a+r, b+r] * c[ix-a, iy-b]         (one rounded product, one rounded sum)
    e = gain * s;  e = e + offset
    readout_noise > 0 only:   e = e + readout_noise * z,   z = sqrt(-2 ln u) * cos(2 pi v)
    frame = clip(rint(e), 0, 2^bits - 1) as uint16                                               (rint: ties to even)

A true convolution with a zero boundary: psf[r+1, r] = 1 moves a count by +1 along x, and charge that spreads past the detector edge
is lost.  The table is used as given, never renormalised: a sum below 1 models a DQE loss.

Random stream.  (u, v) come from Philox-4x32-10 (thermal.philox4x32_10) under the key of the dose, (seed & 0xffffffff, seed >> 32),
with the counter (pixel, p, 0, 1), pixel = ix * my + iy; u = U(x0, x1), v = U(x2, x3) with the U of dose.py.  Word 3 = 1 keeps the
stream apart from the Poisson draws (word 3 = 0).  The frames therefore do not depend on probe_batch.

Without noise the device reproduces every bit: the taps are added in the order above, every product and sum rounds on its own (no
fused multiply-add).  With noise it may differ by one unit where its log / sqrt / cos differ from the host's in the last place AND
e lies that close to a half-integer.

Not built: a correlated or Landau-distributed gain per electron, pixel-to-pixel gain maps, dead pixels, the coincidence loss of
counting mode, and a PSF radius above 8.
"""
from __future__ import annotations

import math

import numpy as np

from .dose import COUNT_MAX, _uniform53
from .thermal import _u64, philox4x32_10

RADIUS_MAX = 8
NOISE_WORD = 1          # word 3 of the counter of the readout noise (the Poisson draws: 0)


def _number(name, v, positive=False):
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not ok or (v <= 0 if positive else v < 0):
        raise ValueError(f"Camera: {name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
    return float(v)


class Camera:
    """The request: psf, None (identity) or a square (2r+1, 2r+1) table of finite weights >= 0 with r <= 8, used as given; gain > 0
    in ADU per electron; offset >= 0 in ADU; readout_noise >= 0, the rms in ADU; bits 1 .. 16, the frame clips at 2^bits - 1;
    keep_counts=True also keeps the electron counts next to the frames."""

    def __init__(self, psf=None, gain=1.0, offset=0.0, readout_noise=0.0, bits=16, keep_counts=False):
        if psf is None:
            table = np.ones((1, 1), dtype=np.float64)
        else:
            try:
                table = np.array(psf, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"Camera: psf must be a square array of numbers, got {psf!r}") from None
            if table.ndim != 2 or table.shape[0] != table.shape[1] or table.shape[0] % 2 != 1:
                raise ValueError(f"Camera: psf must be a square (2r+1, 2r+1) array, got shape {table.shape}")
            if table.shape[0] // 2 > RADIUS_MAX:
                raise ValueError(f"Camera: psf radius {table.shape[0] // 2} is above {RADIUS_MAX}")
            if not np.all(np.isfinite(table)) or np.any(table < 0):
                raise ValueError("Camera: psf entries must be finite and >= 0")
            table = np.where(table == 0, 0.0, table)                # (-0.0 -> +0.0)
        self.psf = np.ascontiguousarray(table)
        self.psf.setflags(write=False)
        self.radius = self.psf.shape[0] // 2
        self.gain = _number("gain", gain, positive=True)
        self.offset = _number("offset", offset)
        self.readout_noise = _number("readout_noise", readout_noise)
        if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, np.integer)) or not 1 <= int(bits) <= 16:
            raise ValueError(f"Camera: bits must be an integer from 1 to 16, got {bits!r}")
        self.bits = int(bits)
        if not isinstance(keep_counts, (bool, np.bool_)):
            raise ValueError(f"Camera: keep_counts must be True or False, got {keep_counts!r}")
        self.keep_counts = bool(keep_counts)

    @property
    def full_scale(self):
        return 2 ** self.bits - 1

    def mtf(self, q):
        """|sum_a (sum_b psf[a+r, b+r]) exp(-2 pi i q a)|: the modulus of the PSF's transform along x at the spatial frequencies q
        (cycles per pixel); mtf(0) is the PSF's sum"""
        q = np.asarray(q, dtype=np.float64)
        a = np.arange(-self.radius, self.radius + 1, dtype=np.float64)
        line = self.psf.sum(axis=1)
        return np.abs((line * np.exp(-2j * np.pi * q[..., None] * a)).sum(axis=-1))

    def __repr__(self):
        return (f"Camera(psf radius {self.radius} sum {float(self.psf.sum()):g}, gain={self.gain:g}, offset={self.offset:g}, "
                f"readout_noise={self.readout_noise:g}, bits={self.bits}" + (", keep_counts=True)" if self.keep_counts else ")"))


def _spread(c, psf):
    """s of the definition for the patterns c (P, mx, my) float64: shifted-array adds, a outer, b inner"""
    r = psf.shape[0] // 2
    P, mx, my = c.shape
    pad = np.zeros((P, mx + 2 * r, my + 2 * r), dtype=np.float64)
    pad[:, r:r + mx, r:r + my] = c
    s = np.zeros(c.shape, dtype=np.float64)
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            s = s + psf[a + r, b + r] * pad[:, r - a:r - a + mx, r - b:r - b + my]          # c[ix - a, iy - b]
    return s


def readout_normals(shape, seed, probe_index):
    """z of the definition for patterns of `shape` = (mx, my) of the probes probe_index (P,) -> (P, mx, my) float64"""
    seed = _u64("seed", seed)
    probes = np.asarray(probe_index).reshape(-1)
    mx, my = int(shape[0]), int(shape[1])
    ctr = np.zeros((probes.size, mx * my, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(mx * my, dtype=np.uint32)[None, :]
    ctr[..., 1] = probes.astype(np.uint32)[:, None]
    ctr[..., 3] = NOISE_WORD
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u, v = _uniform53(x[..., 0], x[..., 1]), _uniform53(x[..., 2], x[..., 3])
    return (np.sqrt(-2.0 * np.log(u)) * np.cos(2.0 * np.pi * v)).reshape(probes.size, mx, my)


def camera_signal(counts, camera, seed, probe_index):
    """e of the definition, before rounding and clipping -> (P, mx, my) float64"""
    if not isinstance(camera, Camera):
        raise ValueError(f"camera_frames: camera must be a Camera object, got {camera!r}")
    c = np.asarray(counts)
    if c.ndim != 3 or c.dtype.kind != "u":
        raise ValueError(f"camera_frames: counts must be (P, mx, my) unsigned integers, got {c.dtype} of shape {c.shape}")
    probes = np.asarray(probe_index).reshape(-1)
    if probes.size != c.shape[0]:
        raise ValueError(f"camera_frames: counts of shape {c.shape} for {probes.size} probes")
    if probes.size and (probes.dtype.kind not in "iu" or probes.min() < 0 or probes.max() > COUNT_MAX):
        raise ValueError("camera_frames: probe indices must be integers in [0, 2^32)")
    if c.shape[1] * c.shape[2] > COUNT_MAX:
        raise ValueError("camera_frames: more than 2^32 - 1 pixels per pattern")
    e = camera.gain * _spread(c.astype(np.float64), camera.psf)
    e = e + camera.offset
    if camera.readout_noise > 0:
        e = e + camera.readout_noise * readout_normals(c.shape[1:], seed, probes)
    return e


def camera_frames(counts, camera, seed, probe_index):
    """The frames of the module's definition -> uint16 (P, mx, my): counts (P, mx, my) unsigned integers, counts[j] the pattern of
    probe probe_index[j] of the scan; seed is the dose's."""
    e = camera_signal(counts, camera, seed, probe_index)
    return np.clip(np.rint(e), 0.0, float(camera.full_scale)).astype(np.uint16)


def electrons(frames, camera):
    """(frames - offset) / gain as float64: the frames read back in electrons"""
    return (np.asarray(frames).astype(np.float64) - camera.offset) / camera.gain


def gaussian_psf(sigma_px, radius=None):
    """(2r+1, 2r+1) samples of a Gaussian of standard deviation sigma_px pixels, normalised to a sum of 1; radius None:
    ceil(3 sigma), at most 8"""
    sigma = _number("sigma_px", sigma_px, positive=True)
    if radius is None:
        radius = min(RADIUS_MAX, int(math.ceil(3.0 * sigma)))
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= RADIUS_MAX:
        raise ValueError(f"gaussian_psf: radius must be an integer from 0 to {RADIUS_MAX}, got {radius!r}")
    a = np.arange(-int(radius), int(radius) + 1, dtype=np.float64)
    g = np.exp(-0.5 * (a / sigma) ** 2)
    table = g[:, None] * g[None, :]
    return table / table.sum()


def psf_from_mtf(mtf, radius):
    """(2r+1, 2r+1) PSF of a radial MTF: mtf, a callable of the spatial frequency in cycles per pixel (0 .. 0.5 along an axis, up to
    0.5 sqrt 2 in the corners of the grid), applied radially: sampled on the (2r+1)^2 DFT grid, inverse transformed, centred, negatives clipped
    to 0, normalised to a sum of 1"""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= RADIUS_MAX:
        raise ValueError(f"psf_from_mtf: radius must be an integer from 0 to {RADIUS_MAX}, got {radius!r}")
    n = 2 * int(radius) + 1
    f = np.fft.fftfreq(n)
    q = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    m = np.asarray(mtf(q), dtype=np.float64)
    if m.shape != q.shape or not np.all(np.isfinite(m)):
        raise ValueError("psf_from_mtf: mtf must return one finite value per frequency")
    table = np.fft.fftshift(np.fft.ifft2(m).real)
    table = np.where(table > 0, table, 0.0)
    total = table.sum()
    if not total > 0:
        raise ValueError("psf_from_mtf: the transform of this mtf has no positive part")
    return table / total

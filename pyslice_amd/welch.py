"""Windowed, segment-averaged (Welch) TACAW spectra: the float64 NumPy definition of what msl_tacaw_welch computes on the device
(pyslice_amd/csrc/tacaw_welch.h), and the host-side rules that go with it.  The role prism.prism_waves plays for PRISM.

For one pixel's time line x[0..T), segment length L, hop (1 <= hop <= L), S = 1 + (T - L) // hop segments (frames past the last
full segment are dropped) and a window w[0..L):

    r_s[n] = x[s hop + n] - x[s hop]
    y_s[n] = g[n] (r_s[n] - mean_n r_s[n]),        g = w sqrt(L / (S sum w^2))
    I[f]   = sum_s | sum_n y_s[n] exp(-2 pi i f n / L) |^2,        I[0] := 0

stored fftshifted along f; frequencies = fftshift(fftfreq(L, dt)).  With L = T, hop = T and a boxcar window this is the
reference's TACAW intensity (tacaw_data.py:89-104); otherwise it is scipy.signal.welch(x, fs=1, window=w, nperseg=L,
noverlap=L - hop, detrend='constant', return_onesided=False, scaling='density') * L outside f = 0.
"""
from __future__ import annotations

import numpy as np

WINDOWS = ("boxcar", "hann", "hamming", "blackman")
_LMIN, _LMAX = 16, 128


def window(name_or_array, L: int) -> np.ndarray:
    """(L,) float64: a named window in its periodic (DFT-even) form, as scipy.signal.get_window gives, or a caller's array of L
    non-negative values with sum w^2 > 0"""
    L = int(L)
    if L < 1:
        raise ValueError(f"window: length must be positive, got {L}")
    if isinstance(name_or_array, str):
        n = 2.0 * np.pi * np.arange(L) / L
        if name_or_array == "boxcar":
            return np.ones(L)
        if name_or_array == "hann":
            return 0.5 - 0.5 * np.cos(n)
        if name_or_array == "hamming":
            return 0.54 - 0.46 * np.cos(n)
        if name_or_array == "blackman":
            # 0.42 - 0.5 + 0.08 rounds to -1.4e-17 at n = 0, where the window is exactly zero: no named window is negative
            return np.maximum(0.42 - 0.5 * np.cos(n) + 0.08 * np.cos(2.0 * n), 0.0)
        raise ValueError(f"window: unknown window {name_or_array!r} (named windows: {', '.join(WINDOWS)}; or an array of {L} values)")
    if name_or_array is None:
        return np.ones(L)
    try:
        w = np.array(name_or_array, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"window: expected a name or an array of {L} floats, got {name_or_array!r}") from None
    if w.shape != (L,):
        raise ValueError(f"window: array of shape {w.shape} for segment length {L}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("window: values must be finite and non-negative")
    if not np.sum(w * w) > 0:
        raise ValueError("window: the window is zero everywhere")
    return w


def segments(T: int, L: int, hop: int) -> int:
    """number of full segments of length L at distance hop in T frames"""
    T, L, hop = int(T), int(L), int(hop)
    if T < 2:
        raise ValueError(f"segments: needs at least 2 frames (got {T})")
    if L < 1 or L > T:
        raise ValueError(f"segments: segment length {L} outside [1, {T}] frames")
    if hop < 1 or hop > L:
        raise ValueError(f"segments: hop {hop} outside [1, {L}]")
    return 1 + (T - L) // hop


def hop_of(L: int, overlap: float) -> int:
    """hop = max(1, L - int(overlap L)) for an overlap fraction in [0, 1)"""
    if isinstance(overlap, (bool, np.bool_)) or not isinstance(overlap, (int, float, np.integer, np.floating)) \
            or not (0.0 <= float(overlap) < 1.0):
        raise ValueError(f"overlap must be a fraction in [0, 1), got {overlap!r}")
    return max(1, int(L) - int(float(overlap) * int(L)))


def supported_lengths():
    """segment lengths with a device kernel: the 2-3-5-7-smooth numbers from 16 to 128 (the lengths of the per-lane time kernel)"""
    out = []
    for n in range(_LMIN, _LMAX + 1):
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            out.append(n)
    return out


def nearest_supported(L: int):
    """(below, above): the nearest supported lengths <= L and >= L (None where there is none)"""
    lens = supported_lengths()
    below = [n for n in lens if n <= L]
    above = [n for n in lens if n >= L]
    return (below[-1] if below else None, above[0] if above else None)


def check_segment(L, T=None, what="segment"):
    """the rules of a segment length, before any device work: an integer with a kernel, at most T frames -> int"""
    if isinstance(L, (bool, np.bool_)) or not isinstance(L, (int, np.integer)):
        raise ValueError(f"{what}: expected an integer segment length, got {L!r}")
    L = int(L)
    if L not in supported_lengths():
        lo, hi = nearest_supported(L)
        near = " and ".join(str(v) for v in (lo, hi) if v is not None)
        raise ValueError(f"{what}: no kernel for segment length {L} (2-3-5-7-smooth lengths {_LMIN} ... {_LMAX}); the nearest supported "
                         f"lengths are {near}")
    if T is not None and L > int(T):
        raise ValueError(f"{what}: segment length {L} exceeds the {int(T)} frames of the trajectory")
    return L


def welch_intensity(wf_PTK, L: int, hop: int, window_="boxcar") -> np.ndarray:
    """float64 (P, L, ...) Welch intensity of complex (P, T, ...) waves along axis 1, fftshifted along the frequency axis"""
    x = np.asarray(wf_PTK).astype(np.complex128)
    if x.ndim < 2:
        raise ValueError(f"welch_intensity: expected (P, T, ...) waves, got shape {x.shape}")
    T = x.shape[1]
    S = segments(T, L, hop)
    w = window(window_, L)
    g = w * np.sqrt(L / (S * np.sum(w * w)))
    g = g.reshape((1, L) + (1,) * (x.ndim - 2))
    out = np.zeros((x.shape[0], L) + x.shape[2:], dtype=np.float64)
    for s in range(S):
        seg = x[:, s * hop:s * hop + L]
        r = seg - seg[:, :1]
        y = g * (r - r.mean(axis=1, keepdims=True))
        out += np.abs(np.fft.fft(y, axis=1)) ** 2
    out[:, 0] = 0.0
    return np.fft.fftshift(out, axes=1)

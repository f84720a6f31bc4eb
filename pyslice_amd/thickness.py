"""Thickness series of the probe-batch modes (MultisliceCalculator(thickness=...)): the detector, polar and pattern signals of
run_detectors() / run_polar() / run_diffraction() at chosen slices of the stack, from ONE scan.

Entry k is the wave after the transmission of slice k and before the propagation that follows it -- the exit wave of the stack
cut after slice k, the definition of `layers=`.  Where `layers=` keeps a full block of spectra per layer,
the thickness series reduces every tapped layer on the device at once (msl_set_layer_reduce) and keeps the
signals only, so device memory grows neither with the number of thicknesses nor with the scan.
"""
from __future__ import annotations

import numpy as np


def _index(k, what):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"thickness: {what} must be an integer, got {k!r}")
    return int(k)


class Thickness:
    """The request: slices=[k, ...] 0-based slice indices, or every=n for the slices n-1, 2n-1, ...; the exit wave is always the
    last entry.  patterns: what run_diffraction() keeps -- "position", the pattern of every probe position and thickness,
    (P, mx, my, L), or "pacbed", only their mean over the probes, (mx, my, L), summed on the device."""

    def __init__(self, slices=None, every=None, patterns="position"):
        if (slices is None) == (every is None):
            raise ValueError("Thickness: give either slices=[...] or every=n")
        if patterns not in ("position", "pacbed"):
            raise ValueError(f"Thickness: patterns must be 'position' or 'pacbed', got {patterns!r}")
        if every is not None:
            every = _index(every, "every")
            if every < 1:
                raise ValueError(f"thickness: every must be a positive slice count, got {every}")
        else:
            try:
                slices = [_index(k, "a slice index") for k in slices]
            except TypeError:
                raise ValueError(f"thickness: slices must be a list of slice indices, got {slices!r}") from None
        self.slices, self.every, self.patterns = slices, every, patterns

    def __repr__(self):
        what = f"every={self.every}" if self.every is not None else f"slices={self.slices}"
        return f"Thickness({what}, patterns={self.patterns!r})"

    def resolve(self, n_slices):
        """the sorted, unique slice indices for a stack of n_slices, n_slices - 1 (the exit wave) last; ValueError for an index
        outside [0, n_slices - 1]"""
        ks = range(self.every - 1, n_slices, self.every) if self.every is not None else self.slices
        out = set()
        for k in ks:
            if not 0 <= k <= n_slices - 1:
                raise ValueError(f"thickness: slice index {k} outside [0, {n_slices - 1}]")
            out.add(k)
        out.discard(n_slices - 1)
        return sorted(out) + [n_slices - 1]


def as_thickness(arg):
    """the `thickness` argument of MultisliceCalculator -> a Thickness (a list means Thickness(slices=list))"""
    if isinstance(arg, Thickness):
        return arg
    if isinstance(arg, (str, bytes)) or not hasattr(arg, "__iter__"):
        raise ValueError(f"thickness: expected a list of slice indices or a Thickness object, got {arg!r}")
    return Thickness(slices=list(arg))


def entry(layer, i):
    """index of entry i (negative from the end) of a layer axis"""
    n = len(layer)
    j = _index(i, "layer")
    if not -n <= j < n:
        raise IndexError(f"layer {i} outside the {n} thickness entries")
    return j % n

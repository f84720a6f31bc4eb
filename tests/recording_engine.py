"""A stand-in for _native.Engine that only records its calls (host tests of the calculator: monkeypatch _native.Engine with it)."""
import numpy as np


class RecordingEngine:
    """Takes the constructor arguments of _native.Engine, keeps every call as (name, args, kwargs) in `calls` (the construction
    itself, as "Engine", in `created`) and answers the reads of the run methods with constant arrays of the right shape."""
    n_layers, device = 1, 0

    def __init__(self, nx, ny, nz, *a, n_probes=1, n_frames=0, frame_batch=1, window=None, k_bin=None, **k):
        self.n_probes, self.n_frames, self.frame_batch = n_probes, n_frames, frame_batch
        self.wx, self.wy = window if window else (nx, ny)
        if k_bin:
            self.wx, self.wy = self.wx // k_bin[0], self.wy // k_bin[1]
        self.created = ("Engine", (nx, ny, nz) + a, dict(n_probes=n_probes, n_frames=n_frames, frame_batch=frame_batch, window=window,
                                                         k_bin=k_bin, **k))
        self.calls = []
        self._F = self._D = 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append((name, a, k))
            P, wx, wy = self.n_probes, self.wx, self.wy
            if name == "diffract":
                return np.ones((k["B"], wx // k["bin"][0], wy // k["bin"][1])) * a[1]
            if name == "coherent_finish":
                return np.full((k["B"], wx // k["bin"][0], wy // k["bin"][1]), 0.25)
            if name == "set_detectors":
                self._D = len(a[1])
            if name == "detect":
                return np.zeros((k["B"], a[1], self._D))
            if name == "tacaw_stream_begin":
                self._F = len(a[1])
            if name == "tacaw_stream_finish":
                return np.zeros((P, wx, wy))
            if name == "intensity":
                return np.zeros((P, self._F, wx, wy), dtype=np.float32)
            if name == "wavefunction_c128":
                return np.zeros((P, a[0] if a and a[0] else self.n_frames, wx, wy), dtype=np.complex128)
            if name == "wavefunction":
                return np.zeros((P, self.n_frames, wx, wy), dtype=np.complex64)
        return call


def _short(v, positions):
    if isinstance(v, np.ndarray):
        if positions is not None and v.ndim == 2 and v.shape[1] == 2:         # probe positions: by their index in the run's list
            return "xy" + str([positions.index(tuple(row)) for row in v.tolist()]).replace(" ", "")
        return v.dtype.str[1:] + str(v.shape).replace(" ", "")
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(_short(x, positions) for x in v) + ")"
    if isinstance(v, (float, np.floating)):
        return f"{float(v):.12g}"
    if v is None or isinstance(v, (bool, int, str, np.integer)):
        return str(v)
    return type(v).__name__


def format_calls(calls, positions=None):
    """One line of text per call: the name, positional arguments reduced to scalars or dtype + shape (an (n, 2) array of probe
    positions to the indices of its rows in `positions`), then the keyword arguments."""
    positions = None if positions is None else [tuple(map(float, p)) for p in positions]
    return [name + "(" + ", ".join([_short(x, positions) for x in a] + [f"{key}={_short(x, positions)}" for key, x in k.items()]) + ")"
            for name, a, k in calls]

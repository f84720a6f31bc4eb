"""ctypes binding of libmslice.so (include/mslice.h) -- the only door to the device.

There is deliberately no CPU fallback: if the shared library is missing or no HIP device is
present every call raises.  The NumPy oracle lives under oracle/ and is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSL_LIB") or os.path.join(_HERE, "libmslice.so")

ABI_VERSION = 3          # include/mslice.h: MSL_ABI_VERSION
MSL_OK, MSL_ERR_INVALID, MSL_ERR_HIP, MSL_ERR_UNSUPPORTED, MSL_ERR_STATE, MSL_ERR_NOMEM = 0, -1, -2, -3, -4, -5
(BUF_PROBES, BUF_EXIT, BUF_POTENTIAL, BUF_TRANSMISSION, BUF_WAVEFUNCTION, BUF_INTENSITY, BUF_FORMFACTOR,
 BUF_STREAM_ACC, BUF_STREAM_S1, BUF_STREAM_S2, BUF_STREAM_REF, BUF_LAYERS, BUF_SMATRIX, BUF_FORMFACTOR_ABS,
 BUF_ABSORPTION, BUF_FORMFACTOR_TDS, BUF_TDS_WEIGHT, BUF_FORMFACTOR_FINITE, BUF_IONIZATION_WEIGHT) = range(19)
TDS_MAX_DETECTORS = 4      # include/mslice.h: msl_set_tds
IONIZATION_MAX_CHANNELS = 8     # include/mslice.h: msl_set_ionization

EXPORTS = [
    "msl_abi_version", "msl_line_kernel_class", "msl_last_error", "msl_create", "msl_destroy", "msl_set_kirkland", "msl_set_slices",
    "msl_set_beam", "msl_resize_probes", "msl_set_probes", "msl_set_aberrations", "msl_upload_probes", "msl_shift_probes",
    "msl_build_potential", "msl_upload_potential", "msl_propagate", "msl_propagate_frame", "msl_tacaw",
    "msl_download", "msl_download_wavefunction_c128", "msl_download_frame", "msl_upload_frame", "msl_buffer_bytes", "msl_result_pitch", "msl_device_ptr", "msl_synchronize",
    "msl_get_counters",
    "msl_reset_counters", "msl_fft2_host",
    "msl_tacaw_spectrum", "msl_tacaw_spectrum_weighted", "msl_tacaw_diffraction", "msl_tacaw_dispersion", "msl_adf",
    "msl_select_batch_slot", "msl_propagate_frames", "msl_frame_batch", "msl_build_potentials",
    "msl_tacaw_stream_begin", "msl_tacaw_stream_push", "msl_tacaw_stream_finish",
    "msl_tacaw_stream_set_reference", "msl_tacaw_stream_finish_range",
    "msl_set_layers", "msl_download_layers_c128", "msl_tacaw_layer",
    "msl_set_detectors", "msl_detect", "msl_spectrum_detect", "msl_diffract",
    "msl_polar_layout", "msl_set_polar", "msl_polar_detect",
    "msl_coherent_reset", "msl_coherent_add", "msl_coherent_finish",
    "msl_dose_reset", "msl_dose_add", "msl_dose_counts",
    "msl_set_camera", "msl_camera_frames", "msl_dose_frames",
    "msl_image_reset", "msl_image_add", "msl_image_download",
    "msl_smatrix_begin", "msl_smatrix_beams", "msl_smatrix_build", "msl_smatrix_probes", "msl_smatrix_probes_cropped",
    "msl_smatrix_end",
    "msl_tacaw_welch_has", "msl_tacaw_welch", "msl_tacaw_welch_layer",
    "msl_set_structure", "msl_build_thermal", "msl_thermal_positions",
    "msl_set_modes", "msl_build_modes", "msl_mode_positions",
    "msl_set_layer_reduce", "msl_layer_fetch", "msl_layer_pacbed_reset", "msl_layer_pacbed_add", "msl_layer_pacbed_download",
    "msl_layer_reduce_bytes",
    "msl_set_tilt", "msl_get_tilt",
    "msl_set_bandlimit", "msl_get_bandlimit",
    "msl_set_absorption",
    "msl_set_tds", "msl_tds_fetch", "msl_tds_reduce",
    "msl_set_ionization", "msl_ionization_fetch", "msl_ionization_reduce",
    "msl_set_projection", "msl_get_projection",
    "msl_set_probe_members", "msl_diffract_members", "msl_dose_add_members",
    "msl_set_adjoint", "msl_adjoint_reset", "msl_adjoint_add", "msl_adjoint_download", "msl_adjoint_step_time", "msl_adjoint_layout",
    "msl_adjoint_positions", "msl_adjoint_positions_rows", "msl_adjoint_positions_time",
    "msl_adjoint_probe_params", "msl_adjoint_probe_params_time",
]
DET_SIGNALS = {"intensity": 0, "amplitude": 1, "com_x": 2, "com_y": 3}      # include/mslice.h: MSL_DET_*
MEMBERS_MAX = 128                                                          # include/mslice.h: MSL_MEMBERS_MAX
POLAR_NONE, POLAR_MAX_BINS = 0xFFFF, 4096                                  # include/mslice.h: MSL_POLAR_*
LR_DETECT, LR_POLAR, LR_DIFFRACT, LR_PACBED = 1, 2, 4, 8                   # include/mslice.h: MSL_LR_*
LR_BYTES_BLOCK, LR_BYTES_TAP, LR_BYTES_STAGING = 0, 1, 2                   # include/mslice.h: MSL_LR_BYTES_*


class MslConfig(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("wavelength", C.c_double), ("sigma", C.c_double),
                ("n_probes", C.c_int32), ("n_frames", C.c_int32), ("device", C.c_int32),
                ("keep_potential", C.c_int32), ("fft_path", C.c_int32),
                ("window_nx", C.c_int32), ("window_ny", C.c_int32), ("launch_timing", C.c_int32),
                ("frame_batch", C.c_int32), ("bin_nx", C.c_int32), ("bin_ny", C.c_int32), ("reserved", C.c_int32 * 1)]


class MslCounters(C.Structure):
    _fields_ = [("slice_steps", C.c_uint64), ("frames", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
                ("ms_potential", C.c_double), ("ms_propagate", C.c_double), ("ms_tacaw", C.c_double),
                ("slice_kernel_launches", C.c_uint64), ("ms_slice_kernels", C.c_double),
                ("row_launches", C.c_uint64), ("ms_row", C.c_double),
                ("col_launches", C.c_uint64), ("ms_col", C.c_double)]


_lib = None


def load():
    """Load libmslice.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `python -m pyslice_amd.build_native`). "
            "pyslice_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    sig = {
        "msl_abi_version": (C.c_int, []),
        "msl_line_kernel_class": (C.c_int, [i32]),
        "msl_last_error": (C.c_char_p, [vp]),
        "msl_create": (C.c_int, [C.POINTER(MslConfig), C.POINTER(vp)]),
        "msl_destroy": (C.c_int, [vp]),
        "msl_set_kirkland": (C.c_int, [vp, vp]),
        "msl_set_slices": (C.c_int, [vp, vp, vp]),
        "msl_set_beam": (C.c_int, [vp, dbl, dbl, dbl]),
        "msl_resize_probes": (C.c_int, [vp, i32]),
        "msl_set_probes": (C.c_int, [vp, dbl, vp, i32]),
        "msl_set_aberrations": (C.c_int, [vp, vp, i32]),
        "msl_set_probe_members": (C.c_int, [vp, dbl, vp, vp, i32]),
        "msl_upload_probes": (C.c_int, [vp, vp, i32]),
        "msl_shift_probes": (C.c_int, [vp, vp, vp, i32]),
        "msl_build_potential": (C.c_int, [vp, vp, vp, i64, i32, i32, i32]),
        "msl_build_potentials": (C.c_int, [vp, vp, vp, i64, i32, i32, i32, i32]),
        "msl_upload_potential": (C.c_int, [vp, vp]),
        "msl_propagate": (C.c_int, [vp]),
        "msl_propagate_frame": (C.c_int, [vp, i32]),
        "msl_tacaw": (C.c_int, [vp, vp, vp, i64, i32, i64]),
        "msl_download": (C.c_int, [vp, C.c_int, vp, C.c_size_t, i64, i64]),
        "msl_download_frame": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "msl_download_wavefunction_c128": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "msl_upload_frame": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "msl_buffer_bytes": (C.c_size_t, [vp, C.c_int]),
        "msl_result_pitch": (i64, [vp, C.c_int]),
        "msl_device_ptr": (vp, [vp, C.c_int]),
        "msl_synchronize": (C.c_int, [vp]),
        "msl_get_counters": (C.c_int, [vp, C.POINTER(MslCounters)]),
        "msl_reset_counters": (C.c_int, [vp]),
        "msl_fft2_host": (C.c_int, [vp, vp, vp, i32, i32]),
        "msl_tacaw_spectrum": (C.c_int, [vp, vp, i64, i64, i64, i64, vp, vp]),
        "msl_tacaw_spectrum_weighted": (C.c_int, [vp, vp, i64, i64, i64, i64, vp, vp]),
        "msl_tacaw_diffraction": (C.c_int, [vp, vp, i64, i64, i64, i64, i64, i64, i64, i64, dbl, vp]),
        "msl_tacaw_dispersion": (C.c_int, [vp, vp, i64, i64, i64, i64, vp, i64, vp]),
        "msl_adf": (C.c_int, [vp, vp, i64, i64, i64, i64, vp, vp]),
        "msl_select_batch_slot": (C.c_int, [vp, i32]),
        "msl_propagate_frames": (C.c_int, [vp, i32, i32]),
        "msl_frame_batch": (C.c_int, [vp]),
        "msl_tacaw_stream_begin": (C.c_int, [vp, i32, i32, vp]),
        "msl_tacaw_stream_push": (C.c_int, [vp, i32, i32, i32]),
        "msl_tacaw_stream_finish": (C.c_int, [vp, vp]),
        "msl_tacaw_stream_set_reference": (C.c_int, [vp, vp, i32]),
        "msl_tacaw_stream_finish_range": (C.c_int, [vp, i32, i32, vp, vp]),
        "msl_set_layers": (C.c_int, [vp, vp, i32]),
        "msl_download_layers_c128": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "msl_tacaw_layer": (C.c_int, [vp, i32]),
        "msl_set_detectors": (C.c_int, [vp, i32, vp, vp, vp, vp]),
        "msl_detect": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, vp]),
        "msl_spectrum_detect": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, vp]),
        "msl_polar_layout": (C.c_int, [vp, i64, i32, vp, vp]),
        "msl_set_polar": (C.c_int, [vp, i32, vp]),
        "msl_polar_detect": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, vp]),
        "msl_diffract": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32, vp]),
        "msl_coherent_reset": (C.c_int, [vp, i64]),
        "msl_coherent_add": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32]),
        "msl_coherent_finish": (C.c_int, [vp, i64, i32, i32, i32, i32, i32, vp]),
        "msl_dose_reset": (C.c_int, [vp, i64, i32, i32]),
        "msl_dose_add": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32]),
        "msl_dose_counts": (C.c_int, [vp, i64, dbl, C.c_uint64, i64, vp, vp]),
        "msl_diffract_members": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
        "msl_dose_add_members": (C.c_int, [vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp]),
        "msl_set_camera": (C.c_int, [vp, i32, vp, dbl, dbl, dbl, i32]),
        "msl_camera_frames": (C.c_int, [vp, vp, i64, i32, i32, C.c_uint64, i64, vp]),
        "msl_dose_frames": (C.c_int, [vp, i64, dbl, C.c_uint64, i64, vp, vp, vp]),
        "msl_image_reset": (C.c_int, [vp, i64]),
        "msl_image_add": (C.c_int, [vp, vp, i64, i64, i64, i32, i32, vp, dbl, dbl, i64, i64]),
        "msl_image_download": (C.c_int, [vp, i64, i64, vp]),
        "msl_smatrix_begin": (C.c_int, [vp, i32, i32, dbl]),
        "msl_smatrix_beams": (C.c_int, [vp, vp]),
        "msl_smatrix_build": (C.c_int, [vp]),
        "msl_smatrix_probes": (C.c_int, [vp, vp, i32, i32]),
        "msl_smatrix_probes_cropped": (C.c_int, [vp, vp, vp, i32, i32]),
        "msl_smatrix_end": (C.c_int, [vp]),
        "msl_tacaw_welch_has": (C.c_int, [i32]),
        "msl_tacaw_welch": (C.c_int, [vp, vp, vp, i64, i32, i64, i32, i32, vp]),
        "msl_tacaw_welch_layer": (C.c_int, [vp, i32, i32, i32, vp]),
        "msl_set_structure": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i32]),
        "msl_build_thermal": (C.c_int, [vp, C.c_uint64, i64, i32]),
        "msl_set_absorption": (C.c_int, [vp, vp, i32]),
        "msl_set_tds": (C.c_int, [vp, vp, i32]),
        "msl_tds_fetch": (C.c_int, [vp, i32, vp]),
        "msl_tds_reduce": (C.c_int, [vp, i32, i32, vp, vp]),
        "msl_set_adjoint": (C.c_int, [vp, i32, dbl, vp]),
        "msl_adjoint_reset": (C.c_int, [vp]),
        "msl_adjoint_add": (C.c_int, [vp, vp, i32, vp, vp]),
        "msl_adjoint_download": (C.c_int, [vp, vp]),
        "msl_adjoint_step_time": (C.c_int, [vp, i32, i32, vp]),
        "msl_adjoint_layout": (C.c_int, [vp, vp, vp]),
        "msl_adjoint_positions": (C.c_int, [vp, vp, vp]),
        "msl_adjoint_positions_rows": (C.c_int64, [vp]),
        "msl_adjoint_positions_time": (C.c_int, [vp, i32, vp]),
        "msl_adjoint_probe_params": (C.c_int, [vp, vp, i32, vp]),
        "msl_adjoint_probe_params_time": (C.c_int, [vp, i32, vp]),
        "msl_set_ionization": (C.c_int, [vp, i32, vp, vp, vp]),
        "msl_ionization_fetch": (C.c_int, [vp, i32, vp]),
        "msl_ionization_reduce": (C.c_int, [vp, i32, i32, vp, vp]),
        "msl_thermal_positions": (C.c_int, [vp, C.c_uint64, i64, vp]),
        "msl_set_modes": (C.c_int, [vp, vp, i64, i32, vp, vp, vp, i32, i32]),
        "msl_build_modes": (C.c_int, [vp, C.c_uint64, i64, i32]),
        "msl_mode_positions": (C.c_int, [vp, C.c_uint64, i64, vp]),
        "msl_set_layer_reduce": (C.c_int, [vp, vp, i32, C.c_uint32, i32, i32]),
        "msl_layer_fetch": (C.c_int, [vp, i64, i32, vp, vp, vp]),
        "msl_layer_pacbed_reset": (C.c_int, [vp]),
        "msl_layer_pacbed_add": (C.c_int, [vp, i64]),
        "msl_layer_pacbed_download": (C.c_int, [vp, vp]),
        "msl_layer_reduce_bytes": (C.c_size_t, [vp, i32]),
        "msl_set_tilt": (C.c_int, [vp, dbl, dbl]),
        "msl_get_tilt": (C.c_int, [vp, vp]),
        "msl_set_bandlimit": (C.c_int, [vp, i32, i32]),
        "msl_get_bandlimit": (C.c_int, [vp, vp]),
        "msl_set_projection": (C.c_int, [vp, i32, i32]),
        "msl_get_projection": (C.c_int, [vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.msl_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {lib.msl_abi_version()}, this binding needs {ABI_VERSION}: rebuild it "
                           "(python -m pyslice_amd.build_native --force)")
    _lib = lib
    return lib


def line_kernel_class(n: int) -> int:
    """2: power-of-two register kernel, 1: direct mixed-radix pass, 0: zero-padded convolution / generic kernel (msl_line_kernel_class)"""
    return int(load().msl_line_kernel_class(int(n)))


def fast_lengths(lo: int = 129, hi: int = 2048):
    """line lengths in [lo, hi] that run on a direct slice-loop kernel"""
    return [n for n in range(int(lo), int(hi) + 1) if line_kernel_class(n) > 0]


def welch_has(L: int) -> bool:
    """is there a device kernel for Welch segment length L (msl_tacaw_welch_has)"""
    return bool(load().msl_tacaw_welch_has(int(L)))


def polar_layout(bins, n_bins):
    """(order, seg) of a bin map (msl_polar_layout; host only, no device): order = the indices of the pixels in a bin, sorted by bin
    and stably within it (uint32), seg (n_bins + 1,) int64 with order[seg[b]:seg[b + 1]] the pixels of bin b"""
    b = np.ascontiguousarray(np.asarray(bins).reshape(-1), dtype=np.uint16)
    order = np.empty(max(b.size, 1), dtype=np.uint32)
    seg = np.empty(max(int(n_bins), 0) + 1, dtype=np.int64)
    rc = load().msl_polar_layout(_ptr(b), b.size, int(n_bins), _ptr(order), _ptr(seg))
    if rc != MSL_OK:
        _raise(rc, (load().msl_last_error(None) or b"msl_polar_layout failed").decode())
    return order[:int(seg[-1])], seg


def _raise(rc, msg):
    if rc == MSL_ERR_INVALID:
        raise ValueError(msg)
    if rc == MSL_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == MSL_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One libmslice handle: one HIP device, one stream, all device buffers of one grid."""

    def __init__(self, nx, ny, nz, dx, dy, dz, wavelength, sigma, n_probes=1, n_frames=0, device=0,
                 keep_potential=False, fft_path=0, window=None, launch_timing=False, frame_batch=1, k_bin=None):
        self._lib = load()
        self._h = C.c_void_p()
        cfg = MslConfig(nx=int(nx), ny=int(ny), nz=int(nz), dx=float(dx), dy=float(dy), dz=float(dz),
                        wavelength=float(wavelength), sigma=float(sigma), n_probes=int(n_probes),
                        n_frames=int(n_frames), device=int(device), keep_potential=int(bool(keep_potential)),
                        fft_path=int(fft_path), window_nx=int(window[0]) if window else 0,
                        window_ny=int(window[1]) if window else 0, launch_timing=int(bool(launch_timing)),
                        frame_batch=int(frame_batch), bin_nx=int(k_bin[0]) if k_bin else 0, bin_ny=int(k_bin[1]) if k_bin else 0)
        rc = self._lib.msl_create(C.byref(cfg), C.byref(self._h))
        if rc != MSL_OK:
            msg = (self._lib.msl_last_error(None) or b"msl_create failed").decode()
            self._h = C.c_void_p()
            _raise(rc, msg)
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.n_probes, self.n_frames, self.device = int(n_probes), int(n_frames), int(device)
        self.keep_potential = bool(keep_potential)
        # stored shape of one exit-wave spectrum: the k-window, or the whole grid, divided by the detector bin
        self.wx = int(window[0]) if window and window[0] else self.nx
        self.wy = int(window[1]) if window and window[1] else self.ny
        if k_bin:
            self.wx //= max(1, int(k_bin[0]))
            self.wy //= max(1, int(k_bin[1]))
        self.intensity_F = 0               # frequency bins of the resident intensity buffer
        self.layers = []                   # slice indices of the intermediate layers (set_layers); the exit wave is the last layer
        self.frame_batch = int(self._lib.msl_frame_batch(self._h))      # frames that share one sequence of launches

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.msl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != MSL_OK:
            _raise(rc, (self._lib.msl_last_error(self._h) or b"libmslice error").decode())

    # -- setup
    def set_kirkland(self, table):
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.size != 103 * 12:
            raise ValueError(f"Kirkland table must hold 103x3x4 values, got shape {t.shape}")
        self._chk(self._lib.msl_set_kirkland(self._h, _ptr(t)))

    def set_absorption(self, u_by_Z=None, absorb=True):
        """absorptive potential (msl_set_absorption; the definition is absorptive.py): u_by_Z = 103 rms widths per Cartesian axis
        (Angstrom), one per atomic number, for every later build_potential / build_potentials; None clears it.  absorb=False keeps
        the Debye-Waller damping alone."""
        if u_by_Z is None:
            self._chk(self._lib.msl_set_absorption(self._h, None, 0))
            return
        u = np.ascontiguousarray(u_by_Z, dtype=np.float64)
        if u.shape != (103,):
            raise ValueError(f"u_by_Z must hold one width per atomic number 1..103, got shape {u.shape}")
        self._chk(self._lib.msl_set_absorption(self._h, _ptr(u), int(bool(absorb))))

    def set_tds(self, member_bits=None, n_det=0):
        """TDS detector signal of the absorptive potential (msl_set_tds; the definition is tds.py): member_bits (nx, ny) uint16 on the
        fftfreq grid, unshifted, bit d = detector d, n_det in 1..4; None clears it.  After set_absorption(.., absorb=True), before the
        build.  Every later slice loop runs on the two-pass loop and leaves the per-slice sums for tds_fetch()."""
        if member_bits is None:
            self._chk(self._lib.msl_set_tds(self._h, None, 0))
            self.n_tds = 0
            return
        b = np.ascontiguousarray(member_bits, dtype=np.uint16)
        if b.shape != (self.nx, self.ny):
            raise ValueError(f"member_bits must be ({self.nx},{self.ny}), got {b.shape}")
        self._chk(self._lib.msl_set_tds(self._h, _ptr(b), int(n_det)))
        self.n_tds = int(n_det)

    def tds_fetch(self, B=None):
        """I[s, p, d] of the last slice loop, (nz, B, n_det) float64: the TDS generated in slice s that lands on detector d, for the
        first B probes (msl_tds_fetch; one wait for the stream)"""
        return self._slice_sums_fetch(self._lib.msl_tds_fetch, getattr(self, "n_tds", 0), B)

    def tds_reduce(self, slice_index=0, reps=1):
        """the TDS reduction alone, of the work buffer the last slice loop left against the weights of one slice (msl_tds_reduce) ->
        (sums (n_probes, n_det) float64, mean device time of one of the `reps` repeats in ms)"""
        return self._slice_sums_reduce(self._lib.msl_tds_reduce, getattr(self, "n_tds", 0), slice_index, reps)

    def _slice_sums_fetch(self, fetch, n, B):
        """(nz, B, n) float64 of the per-slice sums through msl_tds_fetch / msl_ionization_fetch"""
        b = int(B) if B else self.n_probes
        out = np.empty((self.nz, b, n), dtype=np.float64)
        self._chk(fetch(self._h, b, _ptr(out)))
        return out

    def _slice_sums_reduce(self, reduce, n, slice_index, reps):
        """((n_probes, n) float64, ms per repeat) through msl_tds_reduce / msl_ionization_reduce"""
        out = np.empty((self.n_probes, n), dtype=np.float64)
        ms = C.c_double(0.0)
        self._chk(reduce(self._h, int(slice_index), int(reps), _ptr(out), C.byref(ms)))
        return out, float(ms.value)

    def set_ionization(self, channels=None):
        """element maps (msl_set_ionization; the definition is ionization.py): channels = a list of ionization.Ionization (1 to 8), or
        of (Z, width, cross_section) triples; None or an empty list clears it.  Before the build, which then also makes the weight
        stack.  Every later slice loop runs on the two-pass loop and leaves the per-slice sums for ionization_fetch()."""
        if not channels:
            self._chk(self._lib.msl_set_ionization(self._h, 0, None, None, None))
            self.n_ionization = 0
            return
        rows = [(c.Z, c.width, c.cross_section) if hasattr(c, "cross_section") else tuple(c) for c in channels]
        Z = np.ascontiguousarray([r[0] for r in rows], dtype=np.int32)
        w = np.ascontiguousarray([r[1] for r in rows], dtype=np.float64)
        cs = np.ascontiguousarray([r[2] for r in rows], dtype=np.float64)
        self._chk(self._lib.msl_set_ionization(self._h, len(rows), _ptr(Z), _ptr(w), _ptr(cs)))
        self.n_ionization = len(rows)

    def ionization_fetch(self, B=None):
        """I[s, p, e] of the last slice loop, (nz, B, n) float64: the ionisation probability per incident electron of channel e in
        slice s, for the first B probes (msl_ionization_fetch; one wait for the stream)"""
        return self._slice_sums_fetch(self._lib.msl_ionization_fetch, getattr(self, "n_ionization", 0), B)

    def ionization_reduce(self, slice_index=0, reps=1):
        """the ionisation reduction alone, of the work buffer the last slice loop left against the weights of one slice
        (msl_ionization_reduce) -> (sums (n_probes, n) float64, not divided by a norm; mean device time of one repeat in ms)"""
        return self._slice_sums_reduce(self._lib.msl_ionization_reduce, getattr(self, "n_ionization", 0), slice_index, reps)

    def set_adjoint(self, loss_kind=0, epsilon=1e-20, weight=None):
        """gradients (msl_set_adjoint; the definition is adjoint.py): loss_kind = adjoint.LOSSES[...] allocates the wave stack, the
        float64 accumulator (zeroed) and the data of one probe batch and puts the handle on the two-pass loop; 0 switches it off.
        weight: (nx, ny) >= 0 in the detector's (fftshifted) layout, or None."""
        w = None
        if loss_kind and weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float32)
            if w.shape != (self.nx, self.ny):
                raise ValueError(f"weight must be ({self.nx},{self.ny}), got {w.shape}")
        self._chk(self._lib.msl_set_adjoint(self._h, int(loss_kind), float(epsilon), None if w is None else _ptr(w)))

    def adjoint_reset(self):
        """zero the gradient accumulator (msl_adjoint_reset)"""
        self._chk(self._lib.msl_adjoint_reset(self._h))

    def adjoint_add(self, data, B=None, probe=False):
        """the forward loop, the residual against data (B, nx, ny) in the detector's layout and the backward loop for the first B
        probes, added into the accumulator (msl_adjoint_add) -> (loss (B,) float64, probe gradient (B, nx, ny) complex64 or None)"""
        b = int(B) if B else self.n_probes
        d = np.ascontiguousarray(data, dtype=np.float32)
        if d.shape != (b, self.nx, self.ny):
            raise ValueError(f"data must be ({b},{self.nx},{self.ny}), got {d.shape}")
        loss = np.empty(b, dtype=np.float64)
        pg = np.empty((b, self.nx, self.ny), dtype=np.complex64) if probe else None
        self._chk(self._lib.msl_adjoint_add(self._h, _ptr(d), b, _ptr(loss), None if pg is None else _ptr(pg)))
        return loss, pg

    def adjoint_step_time(self, slice_index=0, reps=1):
        """the step kernel of one slice alone over the work buffer the last adjoint_add left (msl_adjoint_step_time) -> mean device
        time of one of the `reps` launches in ms.  It adds into the accumulator: adjoint_reset() afterwards."""
        ms = C.c_double(0.0)
        self._chk(self._lib.msl_adjoint_step_time(self._h, int(slice_index), int(reps), C.byref(ms)))
        return float(ms.value)

    def adjoint_layout(self):
        """(pitch, vec): the row pitch of the work buffer and the wave stack in elements, and whether adjoint_add launches the 16-byte
        variant of the step kernel (msl_adjoint_layout; read-only, for tests)"""
        pitch, vec = C.c_int32(0), C.c_int32(0)
        if self._lib.msl_adjoint_layout(self._h, C.byref(pitch), C.byref(vec)):
            raise RuntimeError("adjoint_layout: no adjoint (set_adjoint)")
        return int(pitch.value), bool(vec.value)

    def adjoint_download(self):
        """the gradient accumulator, (nz, nx, ny) float64 (msl_adjoint_download)"""
        out = np.empty((self.nz, self.nx, self.ny), dtype=np.float64)
        self._chk(self._lib.msl_adjoint_download(self._h, _ptr(out)))
        return out

    def adjoint_positions(self, gamma=None):
        """dL/dr_a of the atoms of the last build_potential, (n_atoms, 3) float64 in the caller's order and axes, the slice-axis column
        zero (msl_adjoint_positions; the definition is adjoint.position_gradient): from gamma (nz, nx, ny) float64 = dL/dV, or from
        the gradient accumulator with gamma=None"""
        g = None
        if gamma is not None:
            g = np.ascontiguousarray(gamma, dtype=np.float64)
            if g.shape != (self.nz, self.nx, self.ny):
                raise ValueError(f"gamma must be ({self.nz},{self.nx},{self.ny}), got {g.shape}")
        n = max(0, int(self._lib.msl_adjoint_positions_rows(self._h)))       # (-1: no build; the call below says which)
        out = np.zeros((max(n, 1), 3), dtype=np.float64)                     # (the handle writes n rows)
        self._chk(self._lib.msl_adjoint_positions(self._h, None if g is None else _ptr(g), _ptr(out)))
        return out[:n]

    def adjoint_positions_time(self, reps=1):
        """the chain of adjoint_positions() on the accumulator alone (msl_adjoint_positions_time) -> mean device time of one of the
        `reps` chains in ms"""
        ms = C.c_double(0.0)
        self._chk(self._lib.msl_adjoint_positions_time(self._h, int(reps), C.byref(ms)))
        return float(ms.value)

    def adjoint_probe_params(self, g0=None, B=None):
        """(B, 30) float64: per probe dL/dx, dL/dy, then the fourteen pairs (dL/da_j, dL/db_j) of its share (msl_adjoint_probe_params;
        the definition is adjoint.probe_parameter_gradient) for the probes the last set_probes built: from g0 (B, nx, ny) complex64 =
        dL/dpsi0*, or with g0=None from the probe gradient the last adjoint_add left in the work buffer"""
        g = None
        if g0 is not None:
            g = np.ascontiguousarray(g0, dtype=np.complex64)
            if g.ndim == 2:
                g = g[None]
            if g.shape[1:] != (self.nx, self.ny) or (B is not None and int(B) != g.shape[0]):
                raise ValueError(f"g0 must be ({'B' if B is None else int(B)},{self.nx},{self.ny}), got {g.shape}")
        b = g.shape[0] if g is not None else (int(B) if B else self.n_probes)
        out = np.zeros((max(b, 1), 30), dtype=np.float64)
        self._chk(self._lib.msl_adjoint_probe_params(self._h, None if g is None else _ptr(g), b, _ptr(out)))
        return out[:b]

    def adjoint_probe_params_time(self, reps=1):
        """the chain of adjoint_probe_params() alone on the work buffer as it stands (msl_adjoint_probe_params_time) -> mean device
        time of one of the `reps` chains in ms"""
        ms = C.c_double(0.0)
        self._chk(self._lib.msl_adjoint_probe_params_time(self._h, int(reps), C.byref(ms)))
        return float(ms.value)

    def set_slices(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self.nz,) or hi.shape != (self.nz,):
            raise ValueError(f"slice edges must have shape ({self.nz},)")
        self._chk(self._lib.msl_set_slices(self._h, _ptr(lo), _ptr(hi)))

    def set_beam(self, wavelength, sigma, dz):
        self._chk(self._lib.msl_set_beam(self._h, float(wavelength), float(sigma), float(dz)))

    def set_tilt(self, tan_x, tan_y):
        """specimen tilt (msl_set_tilt): the tangents of the beam's inclination along x and y.  Every propagator table is rewritten on
        the device, on the handle's stream; the tilt stays on the handle"""
        self._chk(self._lib.msl_set_tilt(self._h, float(tan_x), float(tan_y)))

    def get_tilt(self):
        """(tan_x, tan_y) of the last set_tilt, (0.0, 0.0) before the first (msl_get_tilt)"""
        t = np.zeros(2, dtype=np.float64)
        self._chk(self._lib.msl_get_tilt(self._h, _ptr(t)))
        return float(t[0]), float(t[1])

    def set_bandlimit(self, cut_x, cut_y):
        """band limit (msl_set_bandlimit): keep the frequency indices |h_x| <= cut_x, |h_y| <= cut_y in every propagator table and
        every transmission stack built from now on; (-1, -1) clears it.  bandlimit.BandLimit.cuts() makes the cuts"""
        self._chk(self._lib.msl_set_bandlimit(self._h, int(cut_x), int(cut_y)))

    def get_bandlimit(self):
        """(cut_x, cut_y) of the last set_bandlimit, (-1, -1) without a limit (msl_get_bandlimit)"""
        c = np.zeros(2, dtype=np.int32)
        self._chk(self._lib.msl_get_bandlimit(self._h, _ptr(c)))
        return int(c[0]), int(c[1])

    def set_projection(self, reach_slices, nodes=1):
        """finite projection (msl_set_projection; the definition is projection.py): every later build spreads an atom's potential
        over the reach_slices slices on either side of its own, z resolved on `nodes` planes per slice; reach_slices = 0 turns it off"""
        self._chk(self._lib.msl_set_projection(self._h, int(reach_slices), int(nodes)))

    def get_projection(self):
        """(reach_slices, nodes) of the last set_projection, (0, 1) before the first (msl_get_projection)"""
        c = np.zeros(2, dtype=np.int32)
        self._chk(self._lib.msl_get_projection(self._h, _ptr(c)))
        return int(c[0]), int(c[1])

    def resize_probes(self, n_probes):
        self._chk(self._lib.msl_resize_probes(self._h, int(n_probes)))
        self.n_probes = int(n_probes)

    def set_probes(self, mrad, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self._lib.msl_set_probes(self._h, float(mrad), _ptr(xy), xy.shape[0]))

    def set_probe_members(self, mrad, xy, defocus):
        """set_probes with a defocus (Angstrom, added to the handle's C10) of its own for every probe (msl_set_probe_members): the
        member probes of a partially coherent scan.  All zero: set_probes, bit for bit"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        df = np.ascontiguousarray(defocus, dtype=np.float64).reshape(-1)
        if df.size != xy.shape[0]:
            raise ValueError(f"set_probe_members: {df.size} defocus values for {xy.shape[0]} probes")
        self._chk(self._lib.msl_set_probe_members(self._h, float(mrad), _ptr(xy), _ptr(df), xy.shape[0]))

    def set_aberrations(self, aberrations):
        """aberration function of every later set_probes (msl_set_aberrations): an aberrations.Aberrations, or None to clear.
        Sticky on the handle; upload_probes / shift_probes ignore it"""
        if aberrations is None:
            self._chk(self._lib.msl_set_aberrations(self._h, None, 0))
            return
        polar = np.ascontiguousarray(aberrations.as_polar(), dtype=np.float64)
        if polar.shape != (14, 2):
            raise ValueError(f"aberrations must give (14, 2) polar coefficients, got {polar.shape}")
        self._chk(self._lib.msl_set_aberrations(self._h, _ptr(polar), 14))

    def upload_probes(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.complex64)
        if a.ndim == 2:
            a = a[None]
        if a.shape[1:] != (self.nx, self.ny):
            raise ValueError(f"probe array must be (P,{self.nx},{self.ny}), got {a.shape}")
        self._chk(self._lib.msl_upload_probes(self._h, _ptr(a), a.shape[0]))

    def shift_probes(self, base, xy):
        b = np.ascontiguousarray(base, dtype=np.complex64)
        if b.shape != (self.nx, self.ny):
            raise ValueError(f"base probe must be ({self.nx},{self.ny}), got {b.shape}")
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self._lib.msl_shift_probes(self._h, _ptr(b), _ptr(xy), xy.shape[0]))

    # -- per frame
    def build_potential(self, positions, Z, slice_axis=2):
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError(f"positions must be (n_atoms,3), got {pos.shape}")
        z = np.ascontiguousarray(Z, dtype=np.int32)
        if z.shape != (pos.shape[0],):
            raise ValueError("one atomic number per atom required")
        axes = [0, 1, 2]
        if slice_axis not in axes:
            raise ValueError(f"slice_axis must be 0, 1 or 2, got {slice_axis}")
        axes.remove(slice_axis)
        self._chk(self._lib.msl_build_potential(self._h, _ptr(pos), _ptr(z), pos.shape[0], axes[0], axes[1], slice_axis))

    def build_potentials(self, positions, Z, slice_axis=2):
        """potentials of B = positions.shape[0] frames (B <= frame_batch) into the batch slots 0..B-1, one sequence of launches"""
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        if pos.ndim != 3 or pos.shape[2] != 3:
            raise ValueError(f"positions must be (n_frames,n_atoms,3), got {pos.shape}")
        z = np.ascontiguousarray(Z, dtype=np.int32)
        if z.shape != (pos.shape[1],):
            raise ValueError("one atomic number per atom required")
        axes = [0, 1, 2]
        if slice_axis not in axes:
            raise ValueError(f"slice_axis must be 0, 1 or 2, got {slice_axis}")
        axes.remove(slice_axis)
        self._chk(self._lib.msl_build_potentials(self._h, _ptr(pos), _ptr(z), pos.shape[1], pos.shape[0], axes[0], axes[1], slice_axis))

    # -- frozen phonons (msl_set_structure / msl_build_thermal / msl_thermal_positions; the definition is thermal.py)
    def set_structure(self, positions, Z, sigma, slice_axis=2):
        """the base structure of the configurations, resident on the handle from here on: positions (n_atoms, 3), Z, and the rms
        displacement sigma of every atom along each Cartesian axis"""
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError(f"positions must be (n_atoms,3), got {pos.shape}")
        z = np.ascontiguousarray(Z, dtype=np.int32)
        sg = np.ascontiguousarray(sigma, dtype=np.float64)
        if z.shape != (pos.shape[0],):
            raise ValueError("one atomic number per atom required")
        if sg.shape != (pos.shape[0],):
            raise ValueError("one width per atom required")
        axes = [0, 1, 2]
        if slice_axis not in axes:
            raise ValueError(f"slice_axis must be 0, 1 or 2, got {slice_axis}")
        axes.remove(slice_axis)
        self._structure_atoms = None
        self._chk(self._lib.msl_set_structure(self._h, _ptr(pos), _ptr(z), _ptr(sg), pos.shape[0], axes[0], axes[1], slice_axis))
        self._structure_atoms = pos.shape[0]

    def build_thermal(self, seed, first_config, count=1):
        """potentials of the configurations first_config .. first_config+count-1 of the structure (count <= frame_batch) into the
        batch slots 0..count-1 (the selected slot at a frame batch of 1), their positions generated on the device"""
        self._chk(self._lib.msl_build_thermal(self._h, int(seed), int(first_config), int(count)))

    def thermal_positions(self, seed, config):
        """(n_atoms, 3) float64: the positions the device generates for one configuration"""
        n = getattr(self, "_structure_atoms", None)
        out = np.empty((n or 0, 3), dtype=np.float64)
        self._chk(self._lib.msl_thermal_positions(self._h, int(seed), int(config), _ptr(out) if out.size else None))
        return out

    # -- phonon modes (msl_set_modes / msl_build_modes / msl_mode_positions; the definition is phonons.py)
    def set_modes(self, basis_index, wavevectors, tau, displacements, dynamic=True):
        """the modes that move the resident structure (set_structure first; its sigma is not used by the mode builds): basis_index
        (n_atoms,), wavevectors (M, 3) in cycles / Angstrom, tau (M,) in cycles per frame, displacements (M, n_basis, 3) complex in
        Angstrom; dynamic: a time-coherent record, else independent snapshots"""
        W = np.ascontiguousarray(displacements, dtype=np.complex128)
        if W.ndim != 3 or W.shape[2] != 3:
            raise ValueError(f"displacements must be (n_modes,n_basis,3), got {W.shape}")
        b = np.ascontiguousarray(basis_index, dtype=np.int32)
        q = np.ascontiguousarray(wavevectors, dtype=np.float64)
        t = np.ascontiguousarray(tau, dtype=np.float64)
        if b.ndim != 1:
            raise ValueError(f"basis_index must be (n_atoms,), got {b.shape}")
        if q.shape != (W.shape[0], 3):
            raise ValueError(f"wavevectors must be ({W.shape[0]},3), got {q.shape}")
        if t.shape != (W.shape[0],):
            raise ValueError(f"tau must be ({W.shape[0]},), got {t.shape}")
        self._chk(self._lib.msl_set_modes(self._h, _ptr(b) if b.size else None, b.shape[0], W.shape[1], _ptr(q) if q.size else None,
                                          _ptr(t) if t.size else None, _ptr(W) if W.size else None, W.shape[0], int(bool(dynamic))))

    def build_modes(self, seed, first_frame, count=1):
        """potentials of the frames first_frame .. first_frame+count-1 of the modes (count <= frame_batch) into the batch slots
        0..count-1 (the selected slot at a frame batch of 1), their positions synthesised on the device"""
        self._chk(self._lib.msl_build_modes(self._h, int(seed), int(first_frame), int(count)))

    def mode_positions(self, seed, frame):
        """(n_atoms, 3) float64: the positions the device synthesises for one frame"""
        n = getattr(self, "_structure_atoms", None)
        out = np.empty((n or 0, 3), dtype=np.float64)
        self._chk(self._lib.msl_mode_positions(self._h, int(seed), int(frame), _ptr(out) if out.size else None))
        return out

    def upload_potential(self, V_nz_nx_ny):
        v = np.ascontiguousarray(V_nz_nx_ny, dtype=np.float32)
        if v.shape != (self.nz, self.nx, self.ny):
            raise ValueError(f"potential must be ({self.nz},{self.nx},{self.ny}), got {v.shape}")
        self._chk(self._lib.msl_upload_potential(self._h, _ptr(v)))

    def propagate(self):
        self._chk(self._lib.msl_propagate(self._h))

    def propagate_frame(self, slot):
        self._chk(self._lib.msl_propagate_frame(self._h, int(slot)))

    def select_batch_slot(self, b):
        """transmission stack (0 <= b < frame_batch) the next build_potential / upload_potential fills"""
        self._chk(self._lib.msl_select_batch_slot(self._h, int(b)))

    def propagate_frames(self, first_slot, count):
        """slice loop + exit FFT of the frames in batch slots 0..count-1 -> frame slots first_slot..first_slot+count-1"""
        self._chk(self._lib.msl_propagate_frames(self._h, int(first_slot), int(count)))

    def tacaw(self, src_ptr=None, dst_ptr=None, batch=0, T=0, npix=0):
        self._chk(self._lib.msl_tacaw(self._h, C.c_void_p(src_ptr) if src_ptr else None,
                                      C.c_void_p(dst_ptr) if dst_ptr else None, int(batch), int(T), int(npix)))
        if not src_ptr:
            self.intensity_F = self.n_frames

    @staticmethod
    def _welch_window(window, L):
        """the window argument of msl_tacaw_welch: None (boxcar) or L float64 values"""
        if window is None:
            return None
        w = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
        if w.size != int(L):
            raise ValueError(f"tacaw_welch: window of {w.size} values for segment length {int(L)}")
        return w

    def tacaw_welch(self, L, hop, window=None, src_ptr=None, dst_ptr=None, batch=0, T=0, npix=0):
        """windowed, segment-averaged spectra (msl_tacaw_welch): segments of L frames at distance hop, window = None (boxcar) or L
        non-negative floats.  Pointers as tacaw(): none = the handle's wavefunction buffer into its intensity buffer, (P, L, pitch)"""
        w = self._welch_window(window, L)
        self._chk(self._lib.msl_tacaw_welch(self._h, C.c_void_p(src_ptr) if src_ptr else None, C.c_void_p(dst_ptr) if dst_ptr else None,
                                            int(batch), int(T), int(npix), int(L), int(hop), _ptr(w) if w is not None else None))
        if not src_ptr:
            self.intensity_F = int(L)

    def tacaw_welch_layer(self, layer, L, hop, window=None):
        """msl_tacaw_welch on block `layer` of the layered result into the handle's intensity buffer"""
        w = self._welch_window(window, L)
        self._chk(self._lib.msl_tacaw_welch_layer(self._h, int(layer), int(L), int(hop), _ptr(w) if w is not None else None))
        self.intensity_F = int(L)

    @property
    def n_layers(self):
        return len(self.layers) + 1

    def set_layers(self, slices):
        """record fftshift(fft2(.)) of the waves after the transmission of these slices (strictly increasing, < nz - 1) next to the
        exit wave: the result becomes (L, P, T_local, pitch) with the exit last (msl_set_layers; [] = exit only)"""
        s = np.ascontiguousarray(slices, dtype=np.int32).reshape(-1)
        self._chk(self._lib.msl_set_layers(self._h, _ptr(s) if s.size else None, int(s.size)))
        self.layers = [int(v) for v in s]

    def tacaw_layer(self, layer):
        """msl_tacaw on block `layer` of the layered result into the handle's intensity buffer"""
        self._chk(self._lib.msl_tacaw_layer(self._h, int(layer)))
        self.intensity_F = self.n_frames

    def layers_c128(self, n_frames_used=0):
        """(P, n_frames_used, wx, wy, L) complex128: the reference's WFData array, interleaved and widened on the device"""
        T = int(n_frames_used) if n_frames_used else self.n_frames
        out = np.empty((self.n_probes, T, self.wx, self.wy, self.n_layers), dtype=np.complex128)
        self._chk(self._lib.msl_download_layers_c128(self._h, T, _ptr(out), out.nbytes))
        return out

    # -- thickness series of the probe-batch modes (msl_set_layer_reduce / msl_layer_fetch / msl_layer_pacbed_*)
    def set_layer_reduce(self, slices, what, bin=(1, 1)):
        """reduce the waves after these slices (strictly increasing, < nz - 1) and the exit wave, inside every slice loop, to the
        signals `what` asks for (LR_* bits: detectors, polar bins, patterns of `bin` stored pixels, their sum over the probes); one
        reused block of spectra whatever the number of slices.  [] or what = 0 turns the mode off."""
        s = np.ascontiguousarray(slices, dtype=np.int32).reshape(-1)
        bx, by = int(bin[0]), int(bin[1])
        self._chk(self._lib.msl_set_layer_reduce(self._h, _ptr(s) if s.size else None, int(s.size), int(what), bx, by))
        # (a refused call leaves the handle's mode as it was: so does this mirror)
        on = bool(s.size and what)
        self.reduce_layers, self._lr_what, self._lr_bin = ([int(v) for v in s], int(what), (bx, by)) if on else (None, 0, (1, 1))

    def layer_fetch(self, count, B=None):
        """(det, polar, patterns) of the last slice loop, which ran `count` frames, for the first B probes and every layer, the exit
        last: (L, B, count, D), (L, B, count, n_bins), (L, B, wx/bx, wy/by) float64, None for what set_layer_reduce did not ask for
        (the patterns of a pacbed-only set-up stay on the device).  One wait for the stream."""
        if not getattr(self, "reduce_layers", None):
            raise RuntimeError("layer_fetch: call set_layer_reduce first")
        L, b, n, what = len(self.reduce_layers) + 1, int(B) if B else self.n_probes, int(count), self._lr_what
        bx, by = self._lr_bin
        det = np.empty((L, b, n, getattr(self, "n_detectors", 0)), dtype=np.float64) if what & LR_DETECT else None
        pol = np.empty((L, b, n, getattr(self, "n_polar_bins", 0)), dtype=np.float64) if what & LR_POLAR else None
        pat = np.empty((L, b, self.wx // bx, self.wy // by), dtype=np.float64) if what & LR_DIFFRACT else None
        self._chk(self._lib.msl_layer_fetch(self._h, b, n, *(None if a is None else _ptr(a) for a in (det, pol, pat))))
        return det, pol, pat

    def layer_pacbed_reset(self):
        """zero the (L, wx/bx, wy/by) float64 accumulator of the position-averaged patterns (queued)"""
        self._chk(self._lib.msl_layer_pacbed_reset(self._h))

    def layer_pacbed_add(self, B=None):
        """add the patterns of the first B probes of the last slice loop, layer by layer, into the accumulator (queued)"""
        self._chk(self._lib.msl_layer_pacbed_add(self._h, int(B) if B else 0))

    def layer_pacbed(self):
        """(L, wx/bx, wy/by) float64: the accumulator; waits for the stream"""
        if not getattr(self, "reduce_layers", None):
            raise RuntimeError("layer_pacbed: call set_layer_reduce first")
        bx, by = self._lr_bin
        out = np.empty((len(self.reduce_layers) + 1, self.wx // bx, self.wy // by), dtype=np.float64)
        self._chk(self._lib.msl_layer_pacbed_download(self._h, _ptr(out)))
        return out

    def layer_reduce_bytes(self, which):
        """device bytes of the reduce mode's block, tap buffer or staging area (LR_BYTES_*); 0 while the mode is off"""
        return int(self._lib.msl_layer_reduce_bytes(self._h, int(which)))

    def layers_c64(self):
        """(L, P, n_frames, wx, wy) complex64, dense"""
        return self.download(BUF_LAYERS, np.complex64, (self.n_layers, self.n_probes, self.n_frames, self.wx, self.wy))

    # -- streaming TACAW: accumulate the time->frequency transform for chosen bins, tile of frames by tile of frames
    def tacaw_stream_begin(self, T_total, bins=None):
        b = None if bins is None else np.ascontiguousarray(bins, dtype=np.int32).reshape(-1)
        self._chk(self._lib.msl_tacaw_stream_begin(self._h, int(T_total), 0 if b is None else b.size, _ptr(b) if b is not None else None))
        self._stream_F = int(T_total) if b is None else int(b.size)

    def tacaw_stream_push(self, first_slot, count, t0):
        self._chk(self._lib.msl_tacaw_stream_push(self._h, int(first_slot), int(count), int(t0)))

    def tacaw_stream_set_reference(self, slot=0, ref_ptr=None):
        """frames pushed afterwards are folded as Psi - ref: ref = frame slot `slot` of the ring, or a device (P,K) c64 array"""
        self._chk(self._lib.msl_tacaw_stream_set_reference(self._h, C.c_void_p(int(ref_ptr)) if ref_ptr else None, int(slot)))

    def tacaw_stream_finish_range(self, p0, count, dst_ptr, want_total=True):
        """finish the probes [p0, p0+count) only (frame-sharded runs after the reduce): intensity (count, n_bins, K) f32 into the
        device array at dst_ptr; -> (count, wx, wy) float64 total over all bins (or None)"""
        tot = np.empty((int(count), self.wx, self.wy), dtype=np.float64) if want_total else None
        self._chk(self._lib.msl_tacaw_stream_finish_range(self._h, int(p0), int(count), C.c_void_p(int(dst_ptr)) if dst_ptr else None,
                                                          _ptr(tot) if tot is not None and tot.size else None))
        self.intensity_F = self._stream_F
        return tot

    def tacaw_stream_finish(self, want_total=True):
        """-> (P, wx, wy) float64: sum over ALL frequency bins of the intensity (or None); the selected bins become the
        resident intensity buffer (P, n_bins, wx, wy)"""
        tot = np.empty((self.n_probes, self.wx, self.wy), dtype=np.float64) if want_total else None
        self._chk(self._lib.msl_tacaw_stream_finish(self._h, _ptr(tot) if tot is not None else None))
        self.intensity_F = self._stream_F
        return tot

    # -- reductions over resident results; src = (device pointer, B, F, K[, ld]) or None for the handle's own buffer; ld = pitch
    #    in elements between rows of K pixels (default K; a pointer into a library buffer goes with result_pitch())
    @staticmethod
    def _src(src):
        if src is None:
            return None, 0, 0, 0, 0
        ptr, B, F, K = src[:4]
        ld = src[4] if len(src) > 4 else K
        return C.c_void_p(int(ptr)), int(B), int(F), int(K), int(ld)

    def _bfk(self, src):
        return (self.n_probes, self.intensity_F, self.wx * self.wy) if src is None else tuple(int(v) for v in src[1:4])

    def _rows(self, src, B, rows, first, count):
        """(p, b, rows, k, ld, count) of a call over the slots [first, first+count) of the row axis: src = None is the handle's
        own buffer of `rows` frame slots or frequency bins (B = n_probes or fewer), else _src(src); count = None: to the last"""
        if src is None:
            p, b, k, ld = None, int(B) if B else self.n_probes, self.wx * self.wy, 0
        else:
            p, b, rows, k, ld = self._src(src)
        return p, b, rows, k, ld, (rows - int(first)) if count is None else int(count)

    @staticmethod
    def _mask(mask, K):
        """a boolean mask over k-space as K uint8"""
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if m.size != K:
            raise ValueError(f"mask has {m.size} entries, k-space has {K}")
        return m

    def result_pitch(self, what=BUF_WAVEFUNCTION):
        """pixel pitch of the images of the wavefunction / intensity buffer (>= wx*wy, include/mslice.h: msl_result_pitch)"""
        return int(self._lib.msl_result_pitch(self._h, int(what)))

    def result_view(self, what, typestr, rows=None):
        """DeviceArray of a result buffer as (P, rows, wx, wy) with the library's image pitch in its strides
        (rows: n_frames for the wavefunction, intensity_F for the intensity)"""
        pitch = self.result_pitch(what)
        if rows is None:
            rows = self.n_frames if what == BUF_WAVEFUNCTION else self.intensity_F
        es = int(typestr[2:])
        strides = (rows * pitch * es, pitch * es, self.wy * es, es)
        return DeviceArray(self.device_ptr(what), (self.n_probes, rows, self.wx, self.wy), typestr, owner=self, strides=strides)

    def layers_view(self):
        """DeviceArray of the layered result as (L, P, n_frames, wx, wy) c64 with the library's image pitch in its strides"""
        pitch, es = self.result_pitch(BUF_LAYERS), 8
        T = self.n_frames
        strides = (self.n_probes * T * pitch * es, T * pitch * es, pitch * es, self.wy * es, es)
        return DeviceArray(self.device_ptr(BUF_LAYERS), (self.n_layers, self.n_probes, T, self.wx, self.wy), "<c8", owner=self,
                           strides=strides)

    def tacaw_spectrum(self, mask=None, src=None):
        """(B,F) float64: sum over k of the (masked) intensity."""
        B, F, K = self._bfk(src)
        m = None if mask is None else self._mask(mask, K)
        out = np.empty((B, F), dtype=np.float64)
        p, b, f, k, ld = self._src(src)
        self._chk(self._lib.msl_tacaw_spectrum(self._h, p, b, f, k, ld, _ptr(m) if m is not None else None, _ptr(out)))
        return out

    def tacaw_spectrum_weighted(self, weight, src=None):
        """(B,F) float64: sum over k of weight[k] * intensity (any float mask)."""
        B, F, K = self._bfk(src)
        w = np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
        if w.size != K:
            raise ValueError(f"mask has {w.size} entries, k-space has {K}")
        out = np.empty((B, F), dtype=np.float64)
        p, b, f, k, ld = self._src(src)
        self._chk(self._lib.msl_tacaw_spectrum_weighted(self._h, p, b, f, k, ld, _ptr(w), _ptr(out)))
        return out

    def tacaw_diffraction(self, probes=None, freqs=None, scale=1.0, src=None):
        """(K,) float64: scale * sum of I[b,f,:] over the half-open probe and frequency ranges (None = all)."""
        B, F, K = self._bfk(src)
        b0, b1 = (0, B) if probes is None else probes
        f0, f1 = (0, F) if freqs is None else freqs
        out = np.empty(K, dtype=np.float64)
        p, b, f, k, ld = self._src(src)
        self._chk(self._lib.msl_tacaw_diffraction(self._h, p, b, f, k, ld, int(b0), int(b1), int(f0), int(f1), float(scale), _ptr(out)))
        return out

    def tacaw_dispersion(self, flat_indices, src=None):
        """(B,F,n) float32: I[b,f,idx[i]] for flat k indices kx*ny+ky."""
        B, F, K = self._bfk(src)
        idx = np.ascontiguousarray(flat_indices, dtype=np.int64).reshape(-1)
        out = np.empty((B, F, idx.size), dtype=np.float32)
        p, b, f, k, ld = self._src(src)
        self._chk(self._lib.msl_tacaw_dispersion(self._h, p, b, f, k, ld, _ptr(idx), idx.size, _ptr(out)))
        return out

    def adf(self, mask, src=None):
        """(B,) float64: mean over frames of sum_k mask |Psi|."""
        B, T, K = self._bfk(src)
        m = self._mask(mask, K)
        out = np.empty(B, dtype=np.float64)
        p, b, t, k, ld = self._src(src)
        self._chk(self._lib.msl_adf(self._h, p, b, t, k, ld, _ptr(m), _ptr(out)))
        return out

    # -- STEM detectors (msl_set_detectors / msl_detect)
    def set_detectors(self, member, signals, kxs, kys):
        """member: (wx*wy,) uint16 bitmask per stored pixel (bit d: pixel in detector d); signals: one DET_SIGNALS name or
        number per detector; kxs / kys: the stored k axes (wx and wy floats)"""
        m = np.ascontiguousarray(np.asarray(member).reshape(-1), dtype=np.uint16)
        if m.size != self.wx * self.wy:
            raise ValueError(f"detector mask has {m.size} entries, the stored spectrum has {self.wx * self.wy}")
        sig = np.ascontiguousarray([DET_SIGNALS.get(v, -1) if isinstance(v, str) else int(v) for v in signals], dtype=np.int32)
        kx = np.ascontiguousarray(kxs, dtype=np.float32).reshape(-1)
        ky = np.ascontiguousarray(kys, dtype=np.float32).reshape(-1)
        if kx.size != self.wx or ky.size != self.wy:
            raise ValueError(f"k axes of {kx.size} x {ky.size} values, the stored spectrum is {self.wx} x {self.wy}")
        self._chk(self._lib.msl_set_detectors(self._h, int(sig.size), _ptr(m), _ptr(sig), _ptr(kx), _ptr(ky)))
        self.n_detectors = int(sig.size)

    def detect(self, t0=0, count=None, B=None, src=None):
        """(B, count, n_detectors) float64 detector signals of frame slots [t0, t0+count).  src = None: the handle's own
        wavefunction buffer (B = n_probes or fewer: the first B probes); else (device pointer, B, T, K[, ld]) of a caller's
        complex64 array"""
        p, b, T, k, ld, count = self._rows(src, B, self.n_frames, t0, count)
        out = np.empty((max(b, 0), max(count, 0), getattr(self, "n_detectors", 0)), dtype=np.float64)
        self._chk(self._lib.msl_detect(self._h, p, b, T, k, ld, int(t0), count, _ptr(out)))
        return out

    # -- polar detector (msl_set_polar / msl_polar_detect; the definition is polar_data.py)
    def set_polar(self, bins, n_bins):
        """bins: (wx*wy,) uint16 bin id per stored pixel, POLAR_NONE for a pixel in no bin; n_bins: 1 .. POLAR_MAX_BINS"""
        b = np.ascontiguousarray(np.asarray(bins).reshape(-1), dtype=np.uint16)
        if b.size != self.wx * self.wy:
            raise ValueError(f"bin map has {b.size} entries, the stored spectrum has {self.wx * self.wy}")
        self.n_polar_bins = 0
        self._chk(self._lib.msl_set_polar(self._h, int(n_bins), _ptr(b)))
        self.n_polar_bins = int(n_bins)

    def polar_detect(self, t0=0, count=None, B=None, src=None):
        """(B, count, n_bins) float64: |Psi|^2 summed over the pixels of every bin, frame slots [t0, t0+count).  Source as
        detect(): None is the handle's own wavefunction buffer (B = n_probes or fewer: the first B probes); else (device pointer,
        B, T, K[, ld]) of a caller's complex64 array"""
        p, b, T, k, ld, count = self._rows(src, B, self.n_frames, t0, count)
        out = np.empty((max(b, 0), max(count, 0), getattr(self, "n_polar_bins", 0)), dtype=np.float64)
        self._chk(self._lib.msl_polar_detect(self._h, p, b, T, k, ld, int(t0), count, _ptr(out)))
        return out

    # -- spectrum detectors (msl_spectrum_detect)
    def spectrum_detect(self, f0=0, count=None, B=None, src=None):
        """(B, count, n_detectors) float64: the intensity inside every detector at the frequency bins [f0, f0+count), all detectors
        in one pass.  src = None: the handle's own intensity buffer (after tacaw() / a finished stream; B = n_probes or fewer: the
        first B probes); else (device pointer, B, F, K[, ld]) of a caller's float32 (B, F, K) intensity"""
        p, b, F, k, ld, count = self._rows(src, B, self.intensity_F, f0, count)
        out = np.empty((max(b, 0), max(count, 0), getattr(self, "n_detectors", 0)), dtype=np.float64)
        self._chk(self._lib.msl_spectrum_detect(self._h, p, b, F, k, ld, int(f0), count, _ptr(out)))
        return out

    # -- diffraction patterns (msl_diffract)
    def diffract(self, t0=0, count=None, B=None, bin=(1, 1), src=None):
        """(B, wx/bx, wy/by) float64: |Psi|^2 summed over the frame slots [t0, t0+count) and over every bx x by block of pixels
        (a SUM over the frames: divide by count for the mean).  src = None: the handle's own wavefunction buffer (B = n_probes or
        fewer: the first B probes); else (device pointer, B, T, wx, wy[, ld]) of a caller's complex64 (B, T, wx*wy) array"""
        bx, by = int(bin[0]), int(bin[1])
        wx, wy = (self.wx, self.wy) if src is None else (int(src[3]), int(src[4]))
        p, b, T, k, ld, count = self._rows(None if src is None else (*src[:3], wx * wy, *src[5:]), B, self.n_frames, t0, count)
        ok = bx > 0 and by > 0 and wx > 0 and wy > 0 and wx % bx == 0 and wy % by == 0       # (else the library refuses: no output is read)
        out = np.empty((max(b, 0), wx // bx, wy // by) if ok else (1,), dtype=np.float64)
        self._chk(self._lib.msl_diffract(self._h, p, b, T, k, ld, int(t0), count, wx, wy, bx, by, _ptr(out)))
        return out

    # -- coherent frame sums (msl_coherent_reset / msl_coherent_add / msl_coherent_finish)
    def coherent_reset(self, B=None):
        """size the handle's float64 complex accumulator for B probes (None: n_probes) and zero it"""
        self._coherent_B = 0
        self._chk(self._lib.msl_coherent_reset(self._h, int(B) if B else 0))
        self._coherent_B = int(B) if B else self.n_probes

    def coherent_add(self, t0=0, count=None, B=None, src=None):
        """acc[b, k] += the sum of Psi[b, t, k] over the frame slots [t0, t0+count), every addend widened to float64 first.  Source
        as detect(): None is the handle's own wavefunction buffer (B = n_probes or fewer: the first B probes); else (device
        pointer, B, T, K[, ld]) of a caller's complex64 array.  Queued on the handle's stream."""
        p, b, T, k, ld, count = self._rows(src, B, self.n_frames, t0, count)
        self._chk(self._lib.msl_coherent_add(self._h, p, b, T, k, ld, int(t0), count))

    def coherent_finish(self, n, B=None, bin=(1, 1), shape=None):
        """(B, wx/bx, wy/by) float64: |acc / n|^2 summed over every bx x by block of pixels -- after n frames were added, the
        elastic pattern |<Psi>|^2 on the detector pixels of diffract().  shape = (wx, wy) of the rows that were added (None: the
        handle's stored spectrum); B = None: every probe of the last coherent_reset.  The accumulator is left as it is."""
        bx, by = int(bin[0]), int(bin[1])
        wx, wy = (self.wx, self.wy) if shape is None else (int(shape[0]), int(shape[1]))
        b = int(B) if B else getattr(self, "_coherent_B", 0)
        ok = bx > 0 and by > 0 and wx > 0 and wy > 0 and wx % bx == 0 and wy % by == 0       # (else the library refuses: no output is read)
        out = np.empty((max(b, 0), wx // bx, wy // by) if ok and b > 0 else (1,), dtype=np.float64)
        self._chk(self._lib.msl_coherent_finish(self._h, b, int(n), wx, wy, bx, by, _ptr(out)))
        return out

    # -- finite dose (msl_dose_reset / msl_dose_add / msl_dose_counts)
    def dose_reset(self, B=None, shape=None):
        """size the handle's float64 pattern accumulator for B probes (None: n_probes) of shape = (mx, my) detector pixels (None:
        the stored spectrum) and zero it"""
        mx, my = (self.wx, self.wy) if shape is None else (int(shape[0]), int(shape[1]))
        self._dose_shape = None
        self._chk(self._lib.msl_dose_reset(self._h, int(B) if B else 0, mx, my))
        self._dose_shape = (int(B) if B else self.n_probes, mx, my)

    def dose_add(self, t0=0, count=None, B=None, bin=(1, 1), src=None):
        """accumulator += what diffract() returns for the same arguments, on the device.  Queued on the handle's stream."""
        bx, by = int(bin[0]), int(bin[1])
        wx, wy = (self.wx, self.wy) if src is None else (int(src[3]), int(src[4]))
        p, b, T, k, ld, count = self._rows(None if src is None else (*src[:3], wx * wy, *src[5:]), B, self.n_frames, t0, count)
        self._chk(self._lib.msl_dose_add(self._h, p, b, T, k, ld, int(t0), count, wx, wy, bx, by))

    def dose_counts(self, scale, seed, probe0=0, B=None, keep_intensity=False):
        """(counts (B, mx, my) uint32, acc (B, mx, my) float64 or None): the Poisson draws of acc * scale (dose.poisson_counts with
        the probe indices probe0 .. probe0 + B - 1) and, with keep_intensity, the accumulator itself.  B = None: every probe of the
        last dose_reset."""
        shape = getattr(self, "_dose_shape", None)
        if shape is None:                                           # (the output is sized from the reset this wrapper made)
            raise RuntimeError("dose_counts: no accumulator (call dose_reset)")
        b = int(B) if B else shape[0]
        ok = 0 < b <= shape[0]                                      # (else the library refuses: no output is written)
        dims = (b, shape[1], shape[2]) if ok else (1,)
        counts = np.empty(dims, dtype=np.uint32)
        acc = np.empty(dims, dtype=np.float64) if keep_intensity else None
        self._chk(self._lib.msl_dose_counts(self._h, b, float(scale), int(seed), int(probe0), _ptr(counts),
                                            None if acc is None else _ptr(acc)))
        return counts, acc

    # -- member ensembles (msl_diffract_members / msl_dose_add_members; the definition is coherence.py)
    def diffract_members(self, weights, t0=0, count=None, B=None, bin=(1, 1), src=None):
        """(B / G, wx/bx, wy/by) float64: what diffract() returns for the same arguments with the G = len(weights) member waves of
        every position folded on the device, sum_g weights[g] * pattern[q * G + g].  B counts WAVES (a multiple of G)"""
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        bx, by = int(bin[0]), int(bin[1])
        wx, wy = (self.wx, self.wy) if src is None else (int(src[3]), int(src[4]))
        p, b, T, k, ld, count = self._rows(None if src is None else (*src[:3], wx * wy, *src[5:]), B, self.n_frames, t0, count)
        ok = (bx > 0 and by > 0 and wx > 0 and wy > 0 and wx % bx == 0 and wy % by == 0 and w.size > 0
              and b > 0 and b % w.size == 0)                        # (else the library refuses: no output is read)
        out = np.empty((b // w.size, wx // bx, wy // by) if ok else (1,), dtype=np.float64)
        self._chk(self._lib.msl_diffract_members(self._h, p, b, T, k, ld, int(t0), count, wx, wy, bx, by, int(w.size),
                                                 _ptr(w) if w.size else None, _ptr(out)))
        return out

    def dose_add_members(self, weights, t0=0, count=None, B=None, bin=(1, 1), src=None):
        """accumulator += what diffract_members() returns for the same arguments, on the device; the accumulator was reset for
        B / G positions"""
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        bx, by = int(bin[0]), int(bin[1])
        wx, wy = (self.wx, self.wy) if src is None else (int(src[3]), int(src[4]))
        p, b, T, k, ld, count = self._rows(None if src is None else (*src[:3], wx * wy, *src[5:]), B, self.n_frames, t0, count)
        self._chk(self._lib.msl_dose_add_members(self._h, p, b, T, k, ld, int(t0), count, wx, wy, bx, by, int(w.size),
                                                 _ptr(w) if w.size else None))

    # -- detector response (msl_set_camera / msl_camera_frames / msl_dose_frames)
    def set_camera(self, camera):
        """the camera.Camera whose frames camera_frames() / dose_frames() compute; None clears it.  Nothing else on the handle changes."""
        if camera is None:
            self._chk(self._lib.msl_set_camera(self._h, -1, None, 1.0, 0.0, 0.0, 16))
            return
        psf = np.ascontiguousarray(camera.psf, dtype=np.float64)
        self._chk(self._lib.msl_set_camera(self._h, int(camera.radius), _ptr(psf), float(camera.gain), float(camera.offset),
                                           float(camera.readout_noise), int(camera.bits)))

    def camera_frames(self, counts, seed=0, probe0=0):
        """(B, mx, my) uint16: the device's camera.camera_frames of the caller's counts (B, mx, my) -- any unsigned integers up to
        2^32 - 1 -- for the probes probe0 .. probe0 + B - 1"""
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 3:
            raise ValueError(f"camera_frames: counts must be (B, mx, my), got shape {c.shape}")
        frames = np.empty(c.shape if c.size else (1,), dtype=np.uint16)
        self._chk(self._lib.msl_camera_frames(self._h, _ptr(c) if c.size else None, c.shape[0], c.shape[1], c.shape[2], int(seed), int(probe0),
                                              _ptr(frames)))
        return frames

    def dose_frames(self, scale, seed, probe0=0, B=None, keep_counts=False, keep_intensity=False):
        """(frames (B, mx, my) uint16, counts (B, mx, my) uint32 or None, acc (B, mx, my) float64 or None): dose_counts() followed by
        the camera on the device; the counts and the accumulator are downloaded only when asked for"""
        shape = getattr(self, "_dose_shape", None)
        if shape is None:                                           # (the output is sized from the reset this wrapper made)
            raise RuntimeError("dose_frames: no accumulator (call dose_reset)")
        b = int(B) if B else shape[0]
        ok = 0 < b <= shape[0]                                      # (else the library refuses: no output is written)
        dims = (b, shape[1], shape[2]) if ok else (1,)
        frames = np.empty(dims, dtype=np.uint16)
        counts = np.empty(dims, dtype=np.uint32) if keep_counts else None
        acc = np.empty(dims, dtype=np.float64) if keep_intensity else None
        self._chk(self._lib.msl_dose_frames(self._h, b, float(scale), int(seed), int(probe0), _ptr(frames),
                                            None if counts is None else _ptr(counts), None if acc is None else _ptr(acc)))
        return frames, counts, acc

    # -- images through an objective lens (msl_image_reset / msl_image_add / msl_image_download)
    def image_reset(self, n):
        """size the handle's float64 image accumulator for n images of (nx, ny) and zero it"""
        self._chk(self._lib.msl_image_reset(self._h, int(n)))

    def image_add(self, t0=0, count=None, polar=None, aperture_k=0.0, weight=1.0, first=0, stride=1, B=None, src=None):
        """image[first + b * stride] += weight * the sum over the frame slots [t0, t0+count) of |ifft2(ifftshift(Psi[b, t]) * H)|^2,
        H = A(k) exp(-i chi(k)): polar = the (14, 2) array of Aberrations.as_polar() (None: chi = 0), aperture_k in 1/Angstrom
        (<= 0: none).  Source as detect(): None is the handle's own wavefunction buffer (B = n_probes or fewer: the first B probes);
        else (device pointer, B, T[, ld]) of a caller's complex64 (B, T, nx*ny) array of full-grid spectra.  Queued on the
        handle's stream; consumes the real-space exit waves."""
        p, b, T, _, ld, count = self._rows(None if src is None else (*src[:3], self.nx * self.ny, *src[3:]), B, self.n_frames, t0, count)
        pol = None
        if polar is not None:
            pol = np.ascontiguousarray(polar, dtype=np.float64)
            if pol.shape != (14, 2):
                raise ValueError(f"polar must be (14, 2) coefficients, got {pol.shape}")
        self._chk(self._lib.msl_image_add(self._h, p, b, T, ld, int(t0), count, _ptr(pol) if pol is not None else None, float(aperture_k),
                                          float(weight), int(first), int(stride)))

    def image_download(self, first, n):
        """(n, nx, ny) float64: accumulator images [first, first+n); waits for the stream"""
        out = np.empty((max(int(n), 1), self.nx, self.ny), dtype=np.float64)
        self._chk(self._lib.msl_image_download(self._h, int(first), int(n), _ptr(out)))
        return out

    # -- PRISM: plane-wave S-matrix and probe synthesis (msl_smatrix_*)
    def smatrix_begin(self, interpolation, mrad):
        """enumerate the beams of aperture `mrad` at interpolation (fx, fy) and allocate the S-matrix, (Bm, nx, ny) complex64
        -> Bm"""
        fx, fy = (int(interpolation[0]), int(interpolation[1]))
        self._chk(self._lib.msl_smatrix_begin(self._h, fx, fy, float(mrad)))
        return self.smatrix_beams().shape[0]

    def smatrix_beams(self):
        """(Bm, 2) int32: the signed reciprocal-lattice indices (hx, hy) of the beams, in the order of the S-matrix"""
        n = int(self._lib.msl_smatrix_beams(self._h, None))
        if n < 0:
            _raise(n, "msl_smatrix_beams: call smatrix_begin first")
        out = np.empty((n, 2), dtype=np.int32)
        self._lib.msl_smatrix_beams(self._h, _ptr(out))
        return out

    def smatrix_build(self):
        """propagate every beam through the current potential into the S-matrix (chunks of n_probes beams per slice loop);
        overwrites the probe buffer"""
        self._chk(self._lib.msl_smatrix_build(self._h))

    def smatrix_probes(self, xy, slot):
        """synthesise the exit waves of n_probes probe positions from the S-matrix (exit_waves() downloads them) and write their
        spectra into frame slot `slot`; xy: (n_probes, 2) Angstrom"""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self._lib.msl_smatrix_probes(self._h, _ptr(xy), xy.shape[0], int(slot)))

    def smatrix_probes_cropped(self, dst_engine, xy, slot):
        """the same probes on the cropped (nx / fx, ny / fy) grid of `dst_engine` (an Engine of that grid on this device, with the same
        pixel size and wavelength, n_probes = len(xy), n_frames > 0; it needs no potential): the folded exit waves psi_c[i mod wx,
        j mod wy] = psi_p[i, j] go to its exit_waves() and their spectra -- this engine's smatrix_probes spectra at
        prism.crop_index, value for value -- into its frame slot `slot`.  This engine holds the S-matrix and the aberrations."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._chk(self._lib.msl_smatrix_probes_cropped(self._h, dst_engine._h, _ptr(xy), xy.shape[0], int(slot)))

    def smatrix_end(self):
        """free the S-matrix (close(), set_beam() do the same)"""
        self._chk(self._lib.msl_smatrix_end(self._h))

    def smatrix(self):
        """(Bm, nx, ny) complex64: the S-matrix of the last smatrix_build"""
        return self.download(BUF_SMATRIX, np.complex64, (self.smatrix_beams().shape[0], self.nx, self.ny))

    # -- results
    def buffer_bytes(self, what):
        return int(self._lib.msl_buffer_bytes(self._h, int(what)))

    def device_ptr(self, what):
        return self._lib.msl_device_ptr(self._h, int(what)) or 0

    def download(self, what, dtype, shape, first=0, count=0):
        out = np.empty(shape, dtype=dtype)
        self._chk(self._lib.msl_download(self._h, int(what), _ptr(out), out.nbytes, int(first), int(count)))
        return out

    def probes(self):
        return self.download(BUF_PROBES, np.complex64, (self.n_probes, self.nx, self.ny))

    def exit_waves(self):
        return self.download(BUF_EXIT, np.complex64, (self.n_probes, self.nx, self.ny))

    def potential(self):
        return self.download(BUF_POTENTIAL, np.float32, (self.nz, self.nx, self.ny))

    def transmission(self):
        return self.download(BUF_TRANSMISSION, np.complex64, (self.nz, self.nx, self.ny))

    def wavefunction(self, first=0, count=0):
        n = count if count else self.n_probes
        return self.download(BUF_WAVEFUNCTION, np.complex64, (n, self.n_frames, self.wx, self.wy), first, count)

    def wavefunction_c128(self, n_frames_used=0):
        """(P, n_frames_used, wx, wy) complex128: the reference's result dtype, widened on the device (no host astype)"""
        T = int(n_frames_used) if n_frames_used else self.n_frames
        out = np.empty((self.n_probes, T, self.wx, self.wy), dtype=np.complex128)
        self._chk(self._lib.msl_download_wavefunction_c128(self._h, T, _ptr(out), out.nbytes))
        return out

    def frame(self, slot):
        out = np.empty((self.n_probes, self.wx, self.wy), dtype=np.complex64)
        self._chk(self._lib.msl_download_frame(self._h, int(slot), _ptr(out), out.nbytes))
        return out

    def upload_frame(self, slot, data):
        a = np.ascontiguousarray(data, dtype=np.complex64)
        if a.shape != (self.n_probes, self.wx, self.wy):
            raise ValueError(f"frame must be ({self.n_probes},{self.wx},{self.wy}), got {a.shape}")
        self._chk(self._lib.msl_upload_frame(self._h, int(slot), _ptr(a), a.nbytes))

    def intensity(self, first=0, count=0):
        n = count if count else self.n_probes
        return self.download(BUF_INTENSITY, np.float32, (n, self.intensity_F, self.wx, self.wy), first, count)

    def form_factors(self, n_species):
        return self.download(BUF_FORMFACTOR, np.float32, (n_species, self.nx, self.ny))

    def form_factors_finite(self, n_channels):
        """the channel tables (n_species * (2 R + 1) * J, nx, ny) of the last build under set_projection"""
        return self.download(BUF_FORMFACTOR_FINITE, np.float32, (n_channels, self.nx, self.ny))

    def form_factors_abs(self, n_species):
        """the absorptive tables g of the last build with set_absorption(.., absorb=True)"""
        return self.download(BUF_FORMFACTOR_ABS, np.float32, (n_species, self.nx, self.ny))

    def absorption(self):
        """Omega (nz, nx, ny) of the last build with set_absorption(.., absorb=True)"""
        return self.download(BUF_ABSORPTION, np.float32, (self.nz, self.nx, self.ny))

    def form_factors_tds(self, n_species):
        """the detector-restricted tables g_det (n_det, n_species, nx, ny) of the last build with set_tds"""
        return self.download(BUF_FORMFACTOR_TDS, np.float32, (self.n_tds, n_species, self.nx, self.ny))

    def tds_weight(self):
        """w = 1 - exp(-2 sigma^2 Omega_det), (n_det, nz, nx, ny), of the last build with set_tds"""
        return self.download(BUF_TDS_WEIGHT, np.float32, (self.n_tds, self.nz, self.nx, self.ny))

    def ionization_weight(self):
        """W_e,s, (n, nz, nx, ny), of the last build with set_ionization"""
        return self.download(BUF_IONIZATION_WEIGHT, np.float32, (self.n_ionization, self.nz, self.nx, self.ny))

    def synchronize(self):
        self._chk(self._lib.msl_synchronize(self._h))

    def counters(self) -> dict:
        c = MslCounters()
        self._chk(self._lib.msl_get_counters(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in MslCounters._fields_}

    def reset_counters(self):
        self._chk(self._lib.msl_reset_counters(self._h))

    def fft2(self, arr, direction=+1):
        a = np.ascontiguousarray(arr, dtype=np.complex64)
        if a.ndim == 2:
            a = a[None]
        if a.shape[1:] != (self.nx, self.ny):
            raise ValueError(f"array must be (B,{self.nx},{self.ny}), got {a.shape}")
        out = np.empty_like(a)
        self._chk(self._lib.msl_fft2_host(self._h, _ptr(a), _ptr(out), a.shape[0], int(direction)))
        return out


class DeviceArray:
    """Zero-copy view of a library device buffer for torch (``torch.as_tensor(DeviceArray(...), device='cuda')``)."""

    def __init__(self, ptr, shape, typestr, owner=None, strides=None):
        self._owner = owner
        dense, acc = [], int(typestr[2:])
        for n in reversed(shape):
            dense.append(acc)
            acc *= int(n)
        if strides is not None and tuple(int(v) for v in strides) == tuple(reversed(dense)):
            strides = None                              # C-contiguous: the interface wants None
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2,
                                         "strides": None if strides is None else tuple(int(v) for v in strides)}

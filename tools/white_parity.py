"""White-spectrum parity of the slice-loop passes through the C ABI: white-noise probes through unit-modulus random phase screens
(the Fresnel factor is unit modulus too, so the waves stay white in both spaces through every slice), against the float64 oracle,
per image, per line and per pixel.  tests/test_gpu_white_spectrum.py imports white_case(), the case lists and the bounds; run as
a script it measures every case, on the one-pass kernels and on the generic two-pass loop (fft_path=1), and writes the worst
figures per kernel family.

With tilt=(tan_x, tan_y) the same cases run on the tables msl_set_tilt writes, which are not even in k (P[m] != P[n - m]), against
the float64 definition of pyslice_amd/tilt.py: tests/test_gpu_white_tilt.py imports the TILT_* lists, and the script measures them
into a second report.

output_case() extends the contract to the layer taps (msl_set_layers) and to the stored form of every spectrum -- k-window, detector
bin, frame-batch scatter -- on untilted tables: tests/test_gpu_white_output.py imports the OUT_* lists and tap_layout(), the pure
restatement of which line order, row FFT and column pass a tap takes.

gradient_case() takes it to the slice loop backwards (msl_set_adjoint / msl_adjoint_add): white probes, potentials, data and weights
against pyslice_amd/adjoint.py in float64, the probe gradient, every slice of the accumulator and the loss, under a tilt too:
tests/test_gpu_white_gradient.py imports the GRAD_* lists, tests/test_white_gradient_host.py checks the bounds' margins and what they see.
usage: python tools/white_parity.py [out.txt [tilt_out.txt]], or --tilt-only [tilt_out.txt], or --output-only [output_out.txt], or
--gradient-only [gradient_out.txt]"""
import collections
import functools
import math
import os
import re
import sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import multislice_oracle as orc
from pyslice_amd import _native
from pyslice_amd.tilt import Tilt, propagate_tilted


def _smooth13(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


EV = 100e3
DX = DY = 0.1
DZ = 0.5
TOL_DIRECT, TOL_CONV = 3e-6, 1e-5      # per 2-D transform: the white-noise contract of test_fft2_matches_numpy
LINE_FACTOR, PIXEL_FACTOR = 2.0, 10.0  # a line is a smaller sample of the same error; the largest of ~1e5 Rayleigh errors is ~3.4 rms

# every length of _native.fast_lengths(129, 2048): 99 on the mixed-radix pass, 4 on the power-of-two register kernels
DIRECT_LENGTHS = [135, 140, 144, 147, 150, 160, 168, 175, 180, 189, 192, 196, 200, 210, 216, 224, 225, 240, 250, 252, 256, 270, 280,
                  288, 294, 300, 315, 320, 324, 336, 350, 360, 375, 378, 384, 392, 400, 405, 420, 432, 441, 448, 450, 480, 486, 500,
                  504, 512, 525, 540, 560, 567, 576, 588, 600, 625, 630, 640, 648, 672, 675, 700, 720, 729, 750, 756, 768, 784, 800,
                  810, 840, 864, 896, 900, 960, 972, 1000, 1024, 1050, 1080, 1120, 1134, 1152, 1176, 1200, 1250, 1260, 1280, 1296,
                  1344, 1350, 1400, 1440, 1458, 1500, 1512, 1536, 1568, 1600, 1620, 1680, 1728, 2048]
POW2_LENGTHS = [256, 512, 1024, 2048]
MIXED_LENGTHS = [n for n in DIRECT_LENGTHS if n not in POW2_LENGTHS]

# (nx, ny, nz).  Mixed-radix lengths against 135 lines: a direct cross axis, and 135 is no multiple of the 8- or 16-line tiles.
# nz = 3 starts along y, nz = 2 along x, and the two leave the loop on different axes
MIXED_CASES = [c for n in MIXED_LENGTHS for c in ((n, 135, 3), (135, n, 2))]
# the power-of-two kernels take 16 lines at a time; 2048 x 48 puts the cross axis on a convolution; the square-ish grids are the
# alternating scheme (256 / 1024 on both axes) and the interleaved (512) and paired (2048) work-buffer layouts
POW2_CASES = [(256, 144, 3), (144, 256, 2), (1024, 144, 3), (512, 144, 3), (2048, 48, 3)] + \
             [(nx, ny, nz) for nx, ny in ((256, 256), (1024, 256), (512, 512), (2048, 512)) for nz in (2, 3)]
# every convolution length M at both of its edges, the non-smooth lengths below 192, the generic one-pass kernel
CONV_LENGTHS = [33, 64, 127, 128, 129, 143, 191, 192, 349, 501, 511, 513, 641, 997, 1021, 1023, 1025, 1031, 1792, 2039, 2047, 16, 32]
CONV_CASES = [c for n in CONV_LENGTHS for c in ((n, 37, 3), (37, n, 2))]
# (nx, ny, nz, P): the chunks of 16 probes that share a transmission line, one short of, at and one past two chunks
MANY_PROBE_CASES = [(600, 135, 3, 17), (600, 135, 3, 33), (1024, 144, 3, 17), (1024, 144, 3, 33)]
SINGLE_SLICE_CASES = [(600, 135, 1), (256, 256, 1), (501, 37, 1)]
FRAME_BATCH_CASE = (600, 135, 3)

# ---- tilted tables: tangents of 0.85 px and -0.55 px per slice (DX = 0.1, DZ = 0.5), fractional on both axes, inside 200 mrad
TILT = (0.17, -0.11)
TILT_X, TILT_Y = (0.17, 0.0), (0.0, -0.11)
GENERIC_LENGTHS = [16, 32, 143, 169, 176, 182]
# (nx, ny, nz, tilt).  Every mixed-radix length on both axes, both axes tilted: 135 is mixed itself, the loop stays one-pass
TILT_MIXED_CASES = [c + (TILT,) for c in MIXED_CASES]
# four-step R = 16 / 32 and the 2 R^2 kernel with its split-order table against a mixed cross axis, and paired with each other
# (alternating scheme, interleaved work-buffer order); both axes tilted
TILT_POW2_CASES = [c + (TILT,) for c in [(256, 144, 3), (144, 256, 2), (1024, 144, 3), (144, 1024, 2), (512, 144, 3), (144, 512, 2)] +
                   [(nx, ny, nz) for nx, ny in ((256, 256), (1024, 256), (512, 512)) for nz in (2, 3)]]
# the generic one-pass kernel (lengths below 33, 13-smooth lengths 129..191) on both axes, both tilted, against 135 lines (a partial
# last tile) and 144 (whole tiles); every pair plans the one-pass loop
TILT_GENERIC_CASES = [c + (TILT,) for n in GENERIC_LENGTHS for c in ((n, 135, 3), (135, n, 2), (n, 144, 3), (144, n, 2))]
# the tilt along the direct axis (144) only: the loop stays one-pass, and the untilted axis -- every convolution length of
# CONV_LENGTHS, and the 2048-point wave kernel -- reads the even table and the filter that msl_set_tilt wrote on the device
TILT_CROSS_LENGTHS = [n for n in CONV_LENGTHS if n not in DIRECT_LENGTHS and n >= 33 and not (129 <= n <= 191 and _smooth13(n))] + [2048]
TILT_CROSS_CASES = [c for n in TILT_CROSS_LENGTHS for c in ((n, 144, 3, TILT_Y), (144, n, 2, TILT_X))]
# the tilt along an axis whose one-pass kernel needs an even table: msl_set_tilt moves the loop to the two-pass kernels.  The
# transpose of 2047 x 144 x 2 has three slices: one shift of 0.55 px along a single axis leaves white noise correlated by
# sinc(0.55) = 0.57, so at nz = 2 the float64 definition itself is only 0.93 away from the untilted wave, below the no-op threshold
# of 1 (two propagations: 1.16); the two-pass loop runs the same two kernels per slice whatever nz is
TILT_FALLBACK_CASES = [c + (TILT_X,) for c in ((501, 144, 3), (129, 144, 3), (1025, 144, 3), (2047, 144, 2), (2048, 144, 3))] + \
                      [c + (TILT_Y,) for c in ((144, 501, 3), (144, 129, 3), (144, 1025, 3), (144, 2047, 3), (144, 2048, 3))]
# (nx, ny, nz, tilt, layers): even and odd slices leave their pass on different axes, so the taps after slices 0, 1, 2 run the
# one-pass taps along y and along x, in natural and interleaved line order; 501 x 144 with the tilt along x is the two-pass tap
TILT_LAYER_CASES = [(nx, ny, 4, TILT, (0, 1, 2)) for nx, ny in ((600, 135), (135, 600), (256, 256), (512, 512), (1024, 144), (144, 1024))] + \
                   [(501, 144, 4, TILT_X, (0, 1, 2))]


@functools.lru_cache(maxsize=None)
def _mixed_groups():
    """length -> lanes per line of its mixed-radix kernel, from the instantiation lists of csrc/rowtm_launch.h"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pyslice_amd", "csrc", "rowtm_launch.h")).read()
    out = {}
    for a, b, g in re.findall(r"X\((\d+), (\d+), (\d+)\)", src):
        a, b, g = int(a), int(b), int(g)
        out.setdefault(a * b * (2 if g == 64 else 1), g)
    return out


def axis_under_test(nx, ny):
    """(n, n_other) of the axis a case is about: the other one is a cross axis of 135, 144, 37 or 48 points (x where neither is)"""
    cross = (37, 48, 135, 144)
    if nx in cross and (ny not in cross or ny > nx):
        return ny, nx
    return nx, ny


def family(n, n_other):
    """the kernel family the slice loop runs along an axis of n points with n_other lines (mslice.hip: plan_axis_kind)"""
    if n in POW2_LENGTHS and n_other % 16 == 0:
        return {256: "four-step", 1024: "four-step", 512: "2R^2", 2048: "wave-2K"}[n]
    if _native.line_kernel_class(n) == 1:
        return "mixed G%d" % _mixed_groups()[n]
    if n < 33 or (129 <= n <= 191 and _smooth13(n)):
        return "generic one-pass"
    return "convolution %d" % (256 if n <= 128 else 1024 if n <= 512 else 2048 if n <= 1024 else 4096)


def tolerance(nx, ny):
    """rounding of one 2-D transform: both axes on a direct kernel, or an axis on a padded convolution (two transforms of >= 2n)"""
    return TOL_DIRECT if min(_native.line_kernel_class(nx), _native.line_kernel_class(ny)) >= 1 else TOL_CONV


def two_pass_tolerance(nx, ny):
    """the two-pass loop is the kernel set of test_fft2_matches_numpy and gets its contract: 3e-6 with both lengths 13-smooth,
    1e-5 with a Bluestein line (two transforms of >= 2n)"""
    return TOL_DIRECT if _smooth13(nx) and _smooth13(ny) else TOL_CONV


def bounds(nx, ny, nz, spectrum, layer=None, tol=None):
    """(E_img, E_line, E_pix) bounds: rounding adds in quadrature over the 2 (nz - 1) transforms of the loop, one more for the
    fused spectrum; a single-slice exit wave has no transform and gets one tolerance.  layer = k: the spectrum tapped after the
    transmission of slice k, 2 k transforms of the loop and its own (the exit spectrum is layer nz - 1)"""
    n_t = 2 * (nz - 1) + (1 if spectrum else 0) if layer is None else 2 * layer + 1
    b = (tolerance(nx, ny) if tol is None else tol) * np.sqrt(max(n_t, 1))
    return b, LINE_FACTOR * b, PIXEL_FACTOR * b


def white_input(nx, ny, nz, P, seed=None, frames=1):
    """probes (P, nx, ny) complex64 standard normal; V (frames, nz, nx, ny) float32 with sigma V uniform in [0, 2 pi)"""
    rng = np.random.default_rng((nx * 4099 + ny) * 64 + nz * 8 + P if seed is None else seed)
    probes = (rng.standard_normal((P, nx, ny)) + 1j * rng.standard_normal((P, nx, ny))).astype(np.complex64)
    V = (rng.random((frames, nz, nx, ny)) * (2.0 * np.pi / orc.interaction_sigma(EV))).astype(np.float32)
    return probes, V


def _spectrum(psi):
    return np.fft.fftshift(np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))


def tilt_object(tilt):
    """(tan_x, tan_y) -> the Tilt (mrad) with those tangents; None -> no tilt"""
    return Tilt() if tilt is None else Tilt(math.atan(tilt[0]) * 1e3, math.atan(tilt[1]) * 1e3)


def reference(probes, V, nx, ny, nz, tilt=None, layers=None):
    """float64 exit waves and their fftshifted spectra for one potential V (nz, nx, ny).  tilt = (tan_x, tan_y): the loop is the
    definition of pyslice_amd/tilt.py, on t = exp(i sigma V) of the float32 V widened to float64 as the oracle forms it; plain
    NumPy, nothing of the device.  layers = slice indices: a third result, {k: spectrum of the wave after the transmission of slice k}"""
    if tilt is None and layers is None:
        xs, ys, zs = np.arange(nx) * DX, np.arange(ny) * DY, np.arange(nz) * DZ
        ex = orc.propagate(probes, np.moveaxis(V.astype(np.float64), 0, 2), xs, ys, zs, EV)
        return ex, _spectrum(ex)
    t = np.exp(1j * orc.interaction_sigma(EV) * V.astype(np.float64))
    out = propagate_tilted(probes, t, DX, DY, orc.wavelength(EV), DZ, tilt_object(tilt), layers=layers)
    if layers is None:
        return out, _spectrum(out)
    return out[0], _spectrum(out[0]), {k: _spectrum(w) for k, w in out[1].items()}


def metrics(got, want):
    """worst over the images of (P, nx, ny): E_img = rel-L2 of an image; E_line = largest rel-L2 of a single row or column, over
    that line's reference norm; E_pix = max |got - want| / rms(want)"""
    d = np.abs(np.asarray(got).astype(np.complex128) - want) ** 2
    w = np.abs(want) ** 2
    e_img = np.sqrt(d.sum(axis=(1, 2)) / w.sum(axis=(1, 2))).max()
    e_line = max(np.sqrt(d.sum(axis=2) / w.sum(axis=2)).max(), np.sqrt(d.sum(axis=1) / w.sum(axis=1)).max())
    e_pix = np.sqrt(d.max(axis=(1, 2)) / w.mean(axis=(1, 2))).max()
    return float(e_img), float(e_line), float(e_pix)


def engine(nx, ny, nz, P, n_frames=1, fft_path=0, frame_batch=1, window=None, k_bin=None):
    return _native.Engine(nx, ny, nz, DX, DY, DZ, orc.wavelength(EV), orc.interaction_sigma(EV), n_probes=P, n_frames=n_frames,
                          fft_path=fft_path, frame_batch=frame_batch, window=window, k_bin=k_bin)


@functools.lru_cache(maxsize=1)
def case_data(nx, ny, nz, P):
    """input and float64 reference of a case, computed once for the runs that share it"""
    probes, V = white_input(nx, ny, nz, P)
    return (probes, V) + reference(probes, V[0], nx, ny, nz)


@functools.lru_cache(maxsize=1)
def tilt_case_data(nx, ny, nz, P, tilt, layers):
    """the same input, its float64 reference under the tilt and the untilted one (what a no-op of a tilt would give): each
    (exit, spectrum) or, with layers, (exit, spectrum, {k: spectrum of the tap after slice k})"""
    probes, V = case_data(nx, ny, nz, P)[:2]
    return probes, V, reference(probes, V[0], nx, ny, nz, tilt, layers), reference(probes, V[0], nx, ny, nz, None, layers)


def _rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got).astype(np.complex128) - want) / np.linalg.norm(want))


def _run(eng, nx, ny, nz, P, want_exit, want_spec):
    """propagate() + exit_waves(), then propagate_frame(0) + wavefunction() -> the result dict of white_case and the exit waves"""
    eng.reset_counters()
    eng.propagate()
    got_exit = eng.exit_waves()
    # the one-pass loop moves 16 bytes per pixel and slice-step, the two-pass loop 32 (mslice.hip: count_slice_loop); this call
    # takes no layer tap (no frame slot), which would add its own
    one_pass = eng.counters()["algorithmic_bytes"] == (16 * P + 8) * nz * nx * ny
    eng.propagate_frame(0)
    got_spec = eng.wavefunction()[:, 0]
    return dict(exit=metrics(got_exit, want_exit), spectrum=metrics(got_spec, want_spec), one_pass=one_pass), got_exit


def white_case(nx, ny, nz, P=2, fft_path=0, tilt=None, layers=None, restore=False):
    """propagate() + exit_waves(), then propagate_frame(0) + wavefunction() on the same engine ->
    dict(exit=(E_img, E_line, E_pix), spectrum=(...), one_pass=bool: the loop ran one kernel per slice).
    tilt = (tan_x, tan_y): set_tilt() first, against the tilted float64 reference; adds moved = rel-L2 of the exit waves against the
    UNTILTED reference (about 1.4 for both axes tilted: uncorrelated white fields).
    layers = slice indices: set_layers(), propagate_frame(0), layers_c64(); adds layers = {k: metrics of the tap after slice k},
    layers_moved = {k: rel-L2 against the untilted tap} and layers_untilted = {k: metrics against the untilted tap}.
    restore: set_tilt(0, 0) on the same engine and the whole run again, against the untilted reference -> restored = dict(...)"""
    if tilt is None and layers is None:
        probes, V, want_exit, want_spec = case_data(nx, ny, nz, P)
        flat = None
    else:
        probes, V, want, flat = tilt_case_data(nx, ny, nz, P, tilt, None if layers is None else tuple(layers))
        want_exit, want_spec = want[:2]
    eng = engine(nx, ny, nz, P, fft_path=fft_path)
    try:
        eng.upload_probes(probes)
        eng.upload_potential(V[0])
        if tilt is not None:
            eng.set_tilt(*tilt)
        res, got_exit = _run(eng, nx, ny, nz, P, want_exit, want_spec)
        if flat is not None:
            res["moved"] = _rel_l2(got_exit, flat[0])
        if layers is not None:
            eng.set_layers(list(layers))
            eng.propagate_frame(0)
            got = eng.layers_c64()[:, :, 0]                                     # (L, P, nx, ny): the taps, then the exit
            res["layers"] = {k: metrics(got[i], want[2][k]) for i, k in enumerate(layers)}
            res["layers_untilted"] = {k: metrics(got[i], flat[2][k]) for i, k in enumerate(layers)}
            res["layers_moved"] = {k: _rel_l2(got[i], flat[2][k]) for i, k in enumerate(layers)}
            res["layers_exit"] = metrics(got[len(layers)], want_spec)
        if restore:
            eng.set_tilt(0.0, 0.0)
            res["restored"] = _run(eng, nx, ny, nz, P, *flat[:2])[0]
    finally:
        eng.close()
    return res


def frame_batch_case(nx, ny, nz, P=2):
    """two batch slots with different white potentials through one propagate_frames ->
    (metrics of frame 0, of frame 1, rel-L2 of frame 0 against frame 1's reference)"""
    probes, V = white_input(nx, ny, nz, P, frames=2)
    want = [reference(probes, V[b], nx, ny, nz)[1] for b in range(2)]
    eng = engine(nx, ny, nz, P, n_frames=2, frame_batch=2)
    assert eng.frame_batch == 2
    eng.upload_probes(probes)
    for b in range(2):
        eng.select_batch_slot(b)
        eng.upload_potential(V[b])
    eng.propagate_frames(0, 2)
    got = eng.wavefunction()
    eng.close()
    cross = np.linalg.norm(got[:, 0] - want[1]) / np.linalg.norm(want[1])
    return metrics(got[:, 0], want[0]), metrics(got[:, 1], want[1]), float(cross)


def main(out_path):
    cases = [(c, 2) for c in MIXED_CASES + POW2_CASES + CONV_CASES + SINGLE_SLICE_CASES] + [(c[:3], c[3]) for c in MANY_PROBE_CASES]
    worst, bad = {}, 0
    for (nx, ny, nz), P in cases:
        fam = family(*axis_under_test(nx, ny))
        res = [white_case(nx, ny, nz, P, fft_path=path) for path in (0, 1)]
        line = f"{nx:4d} x {ny:4d} x {nz} P={P:2d} {fam:18s}"
        for name in ("exit", "spectrum"):
            b = bounds(nx, ny, nz, name == "spectrum")
            ok = all(v <= lim for v, lim in zip(res[0][name], b))
            bad += not ok
            line += f" | {name} " + " ".join(f"{v:.2e}" for v in res[0][name]) + f" (two-pass {res[1][name][0]:.2e}; bound {b[0]:.2e})" + ("" if ok else " <-- ABOVE")
            w = worst.setdefault((fam, name), [0.0] * 8)
            for i in range(3):
                w[i] = max(w[i], res[0][name][i])
                w[3 + i] = max(w[3 + i], res[0][name][i] / b[i])
            w[6] = max(w[6], res[1][name][0])
            w[7] += 1
        print(line + ("" if res[0]["one_pass"] else "   (two-pass loop)"), flush=True)
    rows = ["White-spectrum parity of the slice-loop passes (tools/white_parity.py): white-noise probes through unit-modulus random phase",
            "screens against the float64 oracle.  Worst figure of every case of a kernel family (the family of the axis under test; the",
            "cross axis is 135, 144 or 37 points).  E_img: rel-L2 of an image; E_line: largest rel-L2 of a single row or column;",
            "E_pix: max |error| / rms.  'of bound': the largest ratio to the bound of the case, tol sqrt(n_t) x (1, 2, 10) with tol = 3e-6",
            "(direct axes) or 1e-5 (an axis on a padded convolution) per 2-D transform.  two-pass: E_img of the generic two-pass loop",
            "(fft_path=1) on the same input.  The bounds of tests/test_gpu_white_spectrum.py are not taken from this file.", "",
            f"{'family':18s} {'result':8s} {'cases':>5s} {'E_img':>9s} {'E_line':>9s} {'E_pix':>9s}   of bound: img  line   pix   two-pass E_img"]
    for (fam, name), w in sorted(worst.items()):
        rows.append(f"{fam:18s} {name:8s} {int(w[7]):5d} {w[0]:9.2e} {w[1]:9.2e} {w[2]:9.2e}            {w[3]:5.2f} {w[4]:5.2f} {w[5]:5.2f}   {w[6]:9.2e}")
    fb = frame_batch_case(*FRAME_BATCH_CASE)
    rows += ["", "frame_batch = 2, %d x %d x %d, a white potential per batch slot: spectrum of frame 0 %s, frame 1 %s; frame 0 against frame 1's" %
             (FRAME_BATCH_CASE + (" ".join(f"{v:.2e}" for v in fb[0]), " ".join(f"{v:.2e}" for v in fb[1]))),
             f"reference {fb[2]:.2f}", f"{len(cases)} cases, {bad} results above their bound"]
    text = "\n".join(rows) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


def tap_axis(nx, ny, nz, k, one_pass=True):
    """the axis of the pass whose output the tap after slice k reads (mslice.hip: slice_is_transposed): "y" (layer_tap's axis 0),
    "x" (axis 1) or "two-pass" (axis 2).  Two four-step axes alternate so that the last pass runs along y; every other pair
    starts along y"""
    if not one_pass:
        return "two-pass"
    fourstep = lambda n, other: n in (256, 1024) and other % 16 == 0
    along_x = (nz - 1 - k) & 1 if fourstep(nx, ny) and fourstep(ny, nx) else k & 1
    return "x" if along_x else "y"


def tilt_main(out_path):
    """every TILT_* case -> the worst figures per list and kernel family, in the form of main()'s report"""
    worst, bad, n_cases = {}, 0, 0

    def note(key, m, b, ok_extra=True):
        nonlocal bad
        ok = all(v <= lim for v, lim in zip(m, b)) and ok_extra
        bad += not ok
        w = worst.setdefault(key, [0.0] * 7)
        for i in range(3):
            w[i] = max(w[i], m[i])
            w[3 + i] = max(w[3 + i], m[i] / b[i])
        w[6] += 1
        return " ".join(f"{v:.2e}" for v in m) + f" (bound {b[0]:.2e})" + ("" if ok else " <-- ABOVE")

    def fam_of(nx, ny):
        n, other = axis_under_test(nx, ny)
        f = family(n, other)
        return f + (" R=16" if n == 256 else " R=32") if f == "four-step" else f

    lists = (("mixed", TILT_MIXED_CASES, True), ("pow2", TILT_POW2_CASES, True), ("generic", TILT_GENERIC_CASES, True),
             ("even axis", TILT_CROSS_CASES, True), ("fallback", TILT_FALLBACK_CASES, False))
    for lname, cases, want_one_pass in lists:
        for nx, ny, nz, tilt in cases:
            res = white_case(nx, ny, nz, tilt=tilt, restore=not want_one_pass)
            fam = fam_of(nx, ny)
            n_cases += 1
            line = f"{lname:9s} {nx:4d} x {ny:4d} x {nz} tilt {tilt} {fam:18s}"
            loop_ok = res["one_pass"] == want_one_pass and res["moved"] > 1.0
            tol = None if want_one_pass else two_pass_tolerance(nx, ny)
            for name in ("exit", "spectrum"):
                line += f" | {name} " + note((lname, fam, name), res[name], bounds(nx, ny, nz, name == "spectrum", tol=tol), loop_ok)
            if not want_one_pass:
                for name in ("exit", "spectrum"):
                    line += f" | (0, 0) again {name} " + note((lname, fam, "0:" + name), res["restored"][name],
                                                               bounds(nx, ny, nz, name == "spectrum"), res["restored"]["one_pass"])
            print(line + f" | moved {res['moved']:.2f}" + ("" if res["one_pass"] else "   (two-pass loop)"), flush=True)
    for nx, ny, nz, tilt, layers in TILT_LAYER_CASES:
        res = white_case(nx, ny, nz, tilt=tilt, layers=layers)
        n_cases += 1
        line = f"layers    {nx:4d} x {ny:4d} x {nz} tilt {tilt}"
        for k in layers:
            ax = tap_axis(nx, ny, nz, k, res["one_pass"])
            ok = res["layers_moved"][k] > 1.0 if k else all(v <= b for v, b in zip(res["layers_untilted"][0], bounds(nx, ny, nz, True, 0)))
            line += f" | tap {k} ({ax}) " + note(("layers", "tap, two-pass loop" if ax == "two-pass" else "tap, pass along " + ax, "layer"), res["layers"][k],
                                                   bounds(nx, ny, nz, True, k), ok)
        line += " | exit " + note(("layers", "exit of the tapped run", "layer"), res["layers_exit"], bounds(nx, ny, nz, True))
        print(line, flush=True)
    rows = ["White-spectrum parity under specimen tilt (tools/white_parity.py): the cases of white_spectrum_parity.txt on the propagator",
            "tables msl_set_tilt writes for the tangents (0.17, -0.11) -- 0.85 px and -0.55 px per slice, tables that are not even in k --",
            "against the float64 definition of pyslice_amd/tilt.py.  Worst figure of every case of a list and kernel family (the family of",
            "the axis under test; the cross axis is 135 or 144 points).  'even axis': the tilt lies along the 144-point axis only, the",
            "family is that of the UNTILTED axis, which reads the even table and the convolution filter the device wrote.  'fallback': the",
            "tilt lies along an axis whose one-pass kernel needs an even table, the loop runs on the two-pass kernels; '0:' rows are the",
            "same engine after set_tilt(0, 0), one-pass again, against the untilted reference.  'layers': the spectra tapped after slices",
            "0, 1, 2 of 4, by the axis of the pass the tap reads.  E_img, E_line, E_pix and 'of bound' as in white_spectrum_parity.txt:",
            "tol sqrt(n_t) x (1, 2, 10), tol = 3e-6 (direct axes) or 1e-5, n_t = 2 (nz - 1) (+ 1 for a spectrum), 2 k + 1 for the tap after",
            "slice k.  The bounds of tests/test_gpu_white_tilt.py are not taken from this file.", "",
            f"{'list':9s} {'family':24s} {'result':10s} {'cases':>5s} {'E_img':>9s} {'E_line':>9s} {'E_pix':>9s}   of bound: img  line   pix"]
    for (lname, fam, name), w in sorted(worst.items()):
        rows.append(f"{lname:9s} {fam:24s} {name:10s} {int(w[6]):5d} {w[0]:9.2e} {w[1]:9.2e} {w[2]:9.2e}            {w[3]:5.2f} {w[4]:5.2f} {w[5]:5.2f}")
    rows += ["", f"{n_cases} cases, {bad} results above their bound, on the wrong loop or not moved by the tilt"]
    text = "\n".join(rows) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


# ---- layer taps and the windowed, binned output (tests/test_gpu_white_output.py, tests/test_white_output_host.py) ----------------
OutputCase = collections.namedtuple("OutputCase", "nx ny nz P layers window k_bin frame_batch fft_path")


def _oc(nx, ny, nz=4, P=2, layers=None, window=None, k_bin=None, frame_batch=1, fft_path=0):
    """a case of output_case(): every slice but the last is tapped unless layers says otherwise"""
    return OutputCase(nx, ny, nz, P, tuple(range(nz - 1)) if layers is None else tuple(layers), window, k_bin, frame_batch, fft_path)


def output_id(c):
    s = f"{c.nx}x{c.ny}x{c.nz}-P{c.P}"
    s += ("-win%dx%d" % tuple(c.window) if c.window else "") + ("-bin%dx%d" % tuple(c.k_bin) if c.k_bin else "")
    return s + (f"-fb{c.frame_batch}" if c.frame_batch > 1 else "") + ("-two_pass" if c.fft_path else "")


# the grids of TILT_LAYER_CASES without a tilt: the conjugate tables fill_propagator derives on the host.  501 x 144 is then
# one-pass, the tap behind a convolution axis
OUT_UNTILTED_CASES = [_oc(c[0], c[1]) for c in TILT_LAYER_CASES]
# alternating scheme: nz = 5 is the other parity (interleaved order up to k = nz - 3, natural at nz - 2); rp 16 and 32 in one run
# and COL_MULPX on both radices; ny % 32 = 16 sends the tap's column pass to the generic kernel with MUL_VEC
OUT_ALTERNATING_CASES = [_oc(256, 256, 5), _oc(1024, 256), _oc(256, 1024), _oc(256, 144)]
# scheme B, interleaved order between a 512-point axis and a 256 / 1024-point one
OUT_SCHEME_B_CASES = [_oc(512, 256), _oc(256, 512), _oc(1024, 512), _oc(512, 1024)]
OUT_PAIRED_CASES = [_oc(2048, 2048, P=1)]                       # both axes on the wave kernel: the paired-lines gather
OUT_WAVE_NATURAL_CASES = [_oc(2048, 144), _oc(144, 2048)]       # natural order out of the wave kernel
OUT_ROWTM2_CASES = [_oc(1000, 135), _oc(135, 1000)]             # G = 64: one wave per line
OUT_MIXED16_CASES = [_oc(max(n for n, g in _mixed_groups().items() if g == 16), 135)]
# a convolution of every cyclic length M = 256, 1024, 2048, 4096 against 144 lines, on both axes
OUT_CONV_LENGTHS = [127, 501, 997, 1025]
OUT_CONV_CASES = [c for n in OUT_CONV_LENGTHS for c in (_oc(n, 144), _oc(144, n))]
OUT_GENERIC_CASES = [_oc(32, 135), _oc(135, 32), _oc(143, 144), _oc(144, 143)]
# the tapped two-pass loop (slice_loop, begin_timed(2 nz + 2)): generic kernels on both axes, a Bluestein-free pair, power-of-two axes
OUT_TWO_PASS_CASES = [_oc(96, 80, fft_path=1), _oc(45, 63, fft_path=1), _oc(256, 144, fft_path=1), _oc(512, 512, fft_path=1)]
# the other tapped two-pass loop (slice_loop with the split row step, begin_timed(5 nz + 2)) runs while msl_set_tds is on, which needs a built absorptive
# potential: tds_loop_case() below.  Smallest grids: 45 x 63 for either loop (nothing in them depends on the size)
OUT_TDS_LOOP_CASES = [(45, 63, 4)]
OUT_PROBE_CHUNK_CASES = [_oc(600, 135, P=17), _oc(256, 256, P=33)]
OUT_WINDOW_BIN_CASES = [_oc(256, 256, window=(64, 96)),                          # fast column kernel, wy % 32 = 0
                        _oc(256, 256, window=(50, 40)),                          # generic pass
                        _oc(256, 256, k_bin=(4, 4)),
                        _oc(256, 256, window=(64, 96), k_bin=(2, 8)),
                        _oc(1024, 256, window=(256, 64), k_bin=(16, 1)),
                        _oc(600, 135, window=(150, 45), k_bin=(5, 3)),           # generic epilogue
                        _oc(45, 63, window=(15, 21), k_bin=(5, 7), fft_path=1)]  # two-pass
# two batch slots, a white potential each: out_group on the fast column kernel, on the generic pass, and bin_frames regrouping by frame
OUT_FRAME_BATCH_CASES = [_oc(256, 256, frame_batch=2), _oc(600, 135, frame_batch=2),
                         _oc(256, 256, window=(64, 96), k_bin=(2, 8), frame_batch=2)]
OUT_WIDE_CASE = _oc(256, 144)
OUTPUT_LISTS = (("untilted", OUT_UNTILTED_CASES), ("alternating", OUT_ALTERNATING_CASES), ("scheme B", OUT_SCHEME_B_CASES),
                ("paired", OUT_PAIRED_CASES), ("wave natural", OUT_WAVE_NATURAL_CASES), ("rowTM2", OUT_ROWTM2_CASES),
                ("mixed G16", OUT_MIXED16_CASES), ("convolution", OUT_CONV_CASES), ("generic", OUT_GENERIC_CASES),
                ("two-pass", OUT_TWO_PASS_CASES), ("probe chunks", OUT_PROBE_CHUNK_CASES), ("window / bin", OUT_WINDOW_BIN_CASES),
                ("frame batch", OUT_FRAME_BATCH_CASES))

AxisPlan = collections.namedtuple("AxisPlan", "kind base R")


def _plan_M(n):
    """mslice.hip, make_plan: the length of the generic plan, n itself when 13-smooth, else the Bluestein power of two >= 2 n - 1"""
    if _smooth13(n):
        return n
    M = 1
    while M < 2 * n - 1:
        M <<= 1
    return M


def plan_radices(nx, ny, fft_path=0):
    """(Rx, Ry) of msl_create: the four-step radix of the exit / tap column kernel and of the fast row FFT, 0 = the generic kernel"""
    if fft_path:
        return 0, 0
    radix = {1024: 32, 256: 16}
    ry, rx = radix.get(ny, 0), radix.get(nx, 0)
    return (rx if rx and ny % 16 == 0 and ny >= 32 else 0), (ry if ry and nx % (256 // ry) == 0 else 0)


def axis_plan(n, n_other, rfast, want=True):
    """mslice.hip, plan_axis_kind: (kind, base, R) of the one-pass kernel along an axis of n points with n_other lines"""
    base = None
    if not want:
        pass
    elif rfast and n_other % 16 == 0:
        base = "fourstep"
    elif n in (512, 2048) and n_other % 16 == 0:
        base = "two" if n == 512 else "wave2k"
    elif 33 <= n <= 512 and (n <= 128 or n >= 192 or _plan_M(n) != n):
        base = "conv"
    elif 513 <= n <= 1024:
        base = "conv2k"
    elif 1025 <= n <= 2047:
        base = "conv4k"
    elif _plan_M(n) <= 1024:
        base = "generic"
    mixed = want and base not in ("fourstep", "two", "wave2k") and n in _mixed_groups()
    R = {"fourstep": rfast, "two": 16, "conv": 16 if n <= 128 else 32, "wave2k": 32, "conv2k": 32, "conv4k": 32}.get(base, 0)
    return AxisPlan("mixed" if mixed else base, base, R)


def grid_plan(nx, ny, fft_path=0):
    """(plan of x, plan of y, one_pass) as msl_create plans a grid"""
    Rx, Ry = plan_radices(nx, ny, fft_path)
    px, py = axis_plan(nx, ny, Rx, not fft_path), axis_plan(ny, nx, Ry, not fft_path)
    return px, py, px.base is not None and py.base is not None


def tap_layout(nx, ny, nz, k, one_pass=True, window=None, fft_path=0):
    """(axis, order, rp, row_fft, column_pass) of the tap after slice k: the axis of tap_axis(); the line order of the work buffer it
    gathers ("natural", "interleaved" with rp = R' of the reading kernel, "paired"; rp = 0 otherwise); the row FFT and the column
    pass of the tap, "fast" (row_pass_pf / col_pass_kernel) or "generic" (line_fft_kernel).  Restates slice_loop_onepass,
    slice_loop_onepass_b, tap_order and the fast_ok of epilogue_x_pass (mslice.hip)"""
    Rx, Ry = plan_radices(nx, ny, fft_path)
    wx, wy = window if window else (nx, ny)
    windowed = wx != nx or wy != ny
    row_fft = "fast" if Ry else "generic"
    column = "fast" if Rx and ny % 32 == 0 and (not windowed or wy % 32 == 0) else "generic"
    if not one_pass:
        return "two-pass", "natural", 0, row_fft, column
    px, py, planned = grid_plan(nx, ny, fft_path)
    assert planned, "no one-pass plan for this grid"
    interleaves = lambda o: o.kind in ("fourstep", "two")
    if px.kind == "fourstep" and py.kind == "fourstep":                 # slice_loop_onepass: the last pass runs along y, in place
        along_y = not ((nz - 1 - k) & 1)
        order = "interleaved" if k < nz - 2 else "natural"
        rp = 32 if (Rx if along_y else Ry) == 32 else 16
    else:                                                               # slice_loop_onepass_b: even passes along y
        along_y = not (k & 1)
        reader = px if along_y else py
        if px.kind == "wave2k" and py.kind == "wave2k":
            order, rp = "paired", 0
        elif interleaves(px) and interleaves(py):
            order, rp = "interleaved", 32 if reader.R == 32 else 16
        else:
            order, rp = "natural", 0
    return "y" if along_y else "x", order, rp if order == "interleaved" else 0, row_fft, column


def loop_bytes(nx, ny, nz, P, groups, n_taps, wpix, one_pass):
    """algorithmic_bytes of one fused, tapped slice loop of `groups` frames (mslice.hip: count_slice_loop, layer_tap): the one-pass
    loop moves 16 bytes per pixel and slice-step and its tap five images, the two-pass loop 32 and three"""
    npix, images = nx * ny, P * groups
    loop = images * nz * (16 if one_pass else 32) * npix + groups * nz * 8 * npix + images * 16 * npix
    return loop + n_taps * images * (npix * 8 * (5 if one_pass else 3) + wpix * 8)


def stored(spec, nx, ny, window=None, k_bin=None):
    """full fftshifted spectra (..., nx, ny) -> what the engine stores: the k-window [n/2 - w/2, n/2 - w/2 + w) on both axes, then the
    coherent sum of every bx x by block (the definition test_k_bin_is_a_block_sum_of_the_full_spectrum uses)"""
    wx, wy = window if window else (nx, ny)
    bx, by = k_bin if k_bin else (1, 1)
    x0, y0 = nx // 2 - wx // 2, ny // 2 - wy // 2
    win = spec[..., x0:x0 + wx, y0:y0 + wy]
    return win.reshape(win.shape[:-2] + (wx // bx, bx, wy // by, by)).sum(axis=(-3, -1))


@functools.lru_cache(maxsize=1)
def output_data(nx, ny, nz, P, layers, frames):
    """white probes, one white potential per batch slot and per slot the float64 (exit spectrum, {k: tap spectrum}), full size"""
    probes, V = white_input(nx, ny, nz, P, frames=frames)
    return probes, V, [reference(probes, V[b], nx, ny, nz, None, layers)[1:] for b in range(frames)]


def output_case(nx, ny, nz, P=2, layers=(), window=None, k_bin=None, frame_batch=1, fft_path=0, wide=False):
    """one engine, white probes, a white potential per batch slot: set_layers, propagate_frame / propagate_frames, layers_c64() and
    wavefunction(), against the float64 reference cropped to the window and block-summed ->
    dict(taps={(slot, k): (E_img, E_line, E_pix)}, exit={slot: (...)}, exit_is_last_block=bool, bytes=algorithmic_bytes of the loop,
    one_pass=True / False / None (the byte count of the one-pass loop, of the two-pass loop, of neither)).
    frame_batch = 2 adds cross={k or "exit": rel-L2 of slot 0 against slot 1's reference} (about sqrt 2); wide adds
    wide_equal = layers_c128() is the complex64 blocks widened, bit for bit."""
    layers, fb = tuple(layers), int(frame_batch)
    probes, V, want = output_data(nx, ny, nz, P, layers, fb)
    eng = engine(nx, ny, nz, P, n_frames=fb, fft_path=fft_path, frame_batch=fb, window=window, k_bin=k_bin)
    try:
        assert eng.frame_batch == fb
        eng.upload_probes(probes)
        for b in range(fb):
            if fb > 1:
                eng.select_batch_slot(b)
            eng.upload_potential(V[b])
        eng.set_layers(list(layers))
        eng.reset_counters()
        if fb > 1:
            eng.propagate_frames(0, fb)
        else:
            eng.propagate_frame(0)
        got = eng.layers_c64()                                  # (L, P, frames, wx, wy): the taps, then the exit
        got_exit = eng.wavefunction()                           # (P, frames, wx, wy)
        n_bytes = eng.counters()["algorithmic_bytes"]
        got_wide = eng.layers_c128() if wide else None
    finally:
        eng.close()
    wpix = got.shape[-2] * got.shape[-1]
    res = dict(taps={}, exit={}, bytes=int(n_bytes), exit_is_last_block=bool(np.array_equal(got[len(layers)], got_exit)))
    res["one_pass"] = {loop_bytes(nx, ny, nz, P, fb, len(layers), wpix, True): True,
                       loop_bytes(nx, ny, nz, P, fb, len(layers), wpix, False): False}.get(res["bytes"])
    ref = [(stored(w[0], nx, ny, window, k_bin), {k: stored(w[1][k], nx, ny, window, k_bin) for k in layers}) for w in want]
    for b in range(fb):
        for i, k in enumerate(layers):
            res["taps"][(b, k)] = metrics(got[i][:, b], ref[b][1][k])
        res["exit"][b] = metrics(got_exit[:, b], ref[b][0])
    if fb > 1:
        res["cross"] = {k: _rel_l2(got[i][:, 0], ref[1][1][k]) for i, k in enumerate(layers)}
        res["cross"]["exit"] = _rel_l2(got_exit[:, 0], ref[1][0])
    if wide:
        res["wide_equal"] = bool(np.array_equal(got_wide, np.moveaxis(got, 0, -1).astype(np.complex128)))
        res["wide_nonzero"] = float(np.count_nonzero(got_wide)) / got_wide.size
    return res


def tds_loop_bytes(nx, ny, nz, P, n_taps, wpix, n_det=1):
    """algorithmic_bytes of one fused, tapped slice_loop under msl_set_tds (56 bytes per pixel and slice-step, the weights once per slice)"""
    npix = nx * ny
    return P * nz * 56 * npix + nz * 8 * npix + P * 16 * npix + nz * n_det * 4 * npix + n_taps * P * (npix * 8 * 3 + wpix * 8)


def tds_loop_case(nx, ny, nz, P=2, layers=None):
    """the taps of slice_loop under msl_set_tds: msl_set_tds needs an absorptive potential built from atoms, so the stack is a few atoms under
    absorption, downloaded, and the float64 reference runs on the device's own t; the probes are white as everywhere here ->
    dict(taps={k: metrics}, exit=metrics, tds_loop=bool: the byte count is that of the split row step)"""
    import pyslice_amd as ps
    from pyslice_amd.potentials import slice_edges
    layers = tuple(range(nz - 1)) if layers is None else tuple(layers)
    probes = white_input(nx, ny, nz, P)[0]
    rng = np.random.default_rng(nx * 4099 + ny)
    pos = rng.random((12, 3)) * [nx * DX, ny * DY, nz * DZ]
    Z = np.where(np.arange(12) % 2, 14, 8).astype(np.int32)
    eng = engine(nx, ny, nz, P)
    try:
        eng.set_kirkland(ps.loadKirkland())
        eng.set_slices(*slice_edges(np.arange(nz) * DZ))
        eng.set_absorption(np.full(103, 0.08), True)
        eng.set_tds(np.ones((nx, ny), dtype=np.uint16), 1)
        eng.build_potential(pos, Z)
        eng.upload_probes(probes)
        t = eng.transmission().astype(np.complex128)
        eng.set_layers(list(layers))
        eng.reset_counters()
        eng.propagate_frame(0)
        got = eng.layers_c64()[:, :, 0]
        n_bytes = eng.counters()["algorithmic_bytes"]
    finally:
        eng.close()
    ex, taps = propagate_tilted(probes, t, DX, DY, orc.wavelength(EV), DZ, Tilt(), layers=layers)
    return dict(taps={k: metrics(got[i], _spectrum(taps[k])) for i, k in enumerate(layers)}, exit=metrics(got[len(layers)], _spectrum(ex)),
                tds_loop=int(n_bytes) == tds_loop_bytes(nx, ny, nz, P, len(layers), nx * ny), t_range=float(np.abs(t - 1).max()))


def case_bounds(c, k=None):
    """bounds of a tap (k) or of the exit of an OutputCase: the white-noise contract, the two-pass one on the two-pass loop"""
    tol = two_pass_tolerance(c.nx, c.ny) if c.fft_path else None
    return bounds(c.nx, c.ny, c.nz, True, layer=k, tol=tol)


def output_main(out_path):
    """every OUT_* case -> the worst figures per list and tap path, in the form of main()'s report"""
    worst, bad, n_cases = {}, 0, 0

    def note(key, m, b, ok_extra=True):
        nonlocal bad
        ok = all(v <= lim for v, lim in zip(m, b)) and ok_extra
        bad += not ok
        w = worst.setdefault(key, [0.0] * 7)
        for i in range(3):
            w[i] = max(w[i], m[i])
            w[3 + i] = max(w[3 + i], m[i] / b[i])
        w[6] += 1
        return " ".join(f"{v:.2e}" for v in m) + ("" if ok else " <-- ABOVE")

    for lname, cases in OUTPUT_LISTS:
        for c in cases:
            res = output_case(*c)
            n_cases += 1
            line = f"{lname:13s} {output_id(c):44s} one-pass {res['one_pass']}"
            for (b, k), m in sorted(res["taps"].items()):
                lay = tap_layout(c.nx, c.ny, c.nz, k, bool(res["one_pass"]), c.window, c.fft_path)
                path = "tap %s, %s, row %s, column %s" % (lay[0], lay[1] + (f" rp {lay[2]}" if lay[2] else ""), lay[3], lay[4])
                line += f" | slot {b} tap {k} " + note((lname, path), m, case_bounds(c, k), res["one_pass"] == (not c.fft_path))
            for b, m in sorted(res["exit"].items()):
                line += f" | slot {b} exit " + note((lname, "exit"), m, case_bounds(c), res["exit_is_last_block"])
            if "cross" in res:
                bad += not min(res["cross"].values()) > 1.0
                line += " | cross " + " ".join(f"{v:.2f}" for v in res["cross"].values())
            print(line, flush=True)
    for nx, ny, nz in OUT_TDS_LOOP_CASES:
        res = tds_loop_case(nx, ny, nz)
        n_cases += 1
        tol = two_pass_tolerance(nx, ny)
        for k, m in sorted(res["taps"].items()):
            note(("tds loop", "tap two-pass, natural, row generic, column generic"), m, bounds(nx, ny, nz, True, layer=k, tol=tol), res["tds_loop"])
        note(("tds loop", "exit"), res["exit"], bounds(nx, ny, nz, True, tol=tol))
    wide = output_case(*OUT_WIDE_CASE, wide=True)
    bad += not wide["wide_equal"]
    rows = ["White-spectrum parity of the layer taps and the windowed, binned output (tools/white_parity.py --output-only): white-noise",
            "probes through unit-modulus random phase screens, every tap and every stored spectrum against the float64 reference cropped to",
            "the k-window and block-summed.  Worst figure per list and path of the tap (axis of the pass it reads, line order it gathers, row",
            "FFT and column pass of the tap).  E_img, E_line, E_pix and 'of bound' as in white_spectrum_parity.txt: tol sqrt(n_t) x (1, 2, 10),",
            "n_t = 2 k + 1 for the tap after slice k.  The bounds of tests/test_gpu_white_output.py are not taken from this file.", "",
            f"{'list':13s} {'path':58s} {'n':>4s} {'E_img':>9s} {'E_line':>9s} {'E_pix':>9s}   of bound: img  line   pix"]
    for (lname, path), w in sorted(worst.items()):
        rows.append(f"{lname:13s} {path:58s} {int(w[6]):4d} {w[0]:9.2e} {w[1]:9.2e} {w[2]:9.2e}            {w[3]:5.2f} {w[4]:5.2f} {w[5]:5.2f}")
    rows += ["", f"layers_c128() equals the complex64 blocks widened: {wide['wide_equal']} ({output_id(OUT_WIDE_CASE)})",
             f"{n_cases} cases, {bad} results above their bound, on the wrong loop or not separated by batch slot"]
    text = "\n".join(rows) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


# ---- the slice loop backwards (tests/test_gpu_white_gradient.py, tests/test_white_gradient_host.py) -------
# A case: an engine of P probes on the two-pass loop (msl_set_adjoint puts it there), `adds` = the batch sizes of its adjoint_add calls,
# each on P new white probes (the first B of them are used); loss, a white weight or none, a tilt or none.
GradCase = collections.namedtuple("GradCase", "nx ny nz P loss weighted tilt fft_path adds")
GRAD_LOSSES = ("amplitude", "intensity", "poisson")
U_RANGE = 0.5                           # sqrt D = |Psi_ref| (1 + U_RANGE u), u uniform in [-1, 1]
KAPPA_CAP = 4.0                         # the condition on the inputs: kappa_loss of every case and probe
F32_ULP = 2.0 ** -24


def _gcase(nx, ny, nz, P=2, loss="amplitude", weighted=False, tilt="auto", fft_path=0, adds=None):
    """a case of gradient_case(): the tilt TILT on every grid with a propagator (nz > 1) unless tilt says otherwise"""
    tilt = (TILT if nz > 1 else None) if tilt == "auto" else tilt
    return GradCase(nx, ny, nz, P, loss, bool(weighted), tilt, fft_path, (P,) if adds is None else tuple(adds))


def gradient_id(c):
    s = f"{c.nx}x{c.ny}x{c.nz}-P{c.P}-{c.loss}" + ("-w" if c.weighted else "") + ("-tilt" if c.tilt else "")
    return s + ("-two_pass" if c.fft_path else "") + ("" if c.adds == (c.P,) else "-adds" + "+".join(map(str, c.adds)))


# one partial tile in the residual pass (480 of 1024 pixels) and in the step (240 of 512 pairs); nz = 1: no propagator, no stack
GRAD_SINGLE_TILE_CASES = [_gcase(24, 20, 1)]
# 45 x 63 (fft_path=1: pitch 63, the 8-byte step, 2.8 step tiles, odd lengths in the shift mapping of both axes) and 101 x 97 (pitch
# 114: the 16-byte step with its pad pixel and the 8-byte tail store): every loss, the white weight, the tilt
GRAD_ODD_CASES = [_gcase(45, 63, 3, loss=l, weighted=True, fft_path=1) for l in GRAD_LOSSES] + \
                 [_gcase(101, 97, 3, loss=l, weighted=True) for l in GRAD_LOSSES]
# generic lines; the fast row kernel on either axis; 525 pairs per row: the boundaries of the 512-pair tiles fall inside rows
GRAD_GRID_CASES = [_gcase(96, 80, 4), _gcase(256, 64, 2), _gcase(64, 256, 3), _gcase(12, 1050, 2)]
# P = 3: a full add, new probes, a ragged add of 2 on the P-strided stack behind it; P = 1: no prefetch of a next image in flight
GRAD_BATCH_CASES = [_gcase(45, 63, 3, P=3, weighted=True, fft_path=1, adds=(3, 2)), _gcase(101, 97, 3, P=3, weighted=True, adds=(3, 2)),
                    _gcase(45, 63, 3, P=1, weighted=True, fft_path=1), _gcase(101, 97, 3, P=1, weighted=True)]
GRAD_RESTORE_CASE = _gcase(101, 97, 3, weighted=True)           # then set_tilt(0, 0) on the same handle, against the untilted case
GRADIENT_LISTS = (("single tile", GRAD_SINGLE_TILE_CASES), ("odd grids", GRAD_ODD_CASES), ("grids", GRAD_GRID_CASES),
                  ("batches", GRAD_BATCH_CASES))


def step_layout(nx, ny, fft_path=0):
    """(pitch, vec) of msl_adjoint_add on a grid: mslice.hip's pitch (ny, + 16 where a fast kernel or the one-pass loop is planned,
    then even on a one-pass plan) and the 16-byte step on an even pitch (the buffers are on 16 bytes)"""
    Rx, Ry = plan_radices(nx, ny, fft_path)
    pitch = ny + (16 if Rx or Ry else 0)
    if grid_plan(nx, ny, fft_path)[2]:
        pitch = ny + 16 if pitch == ny else pitch
        pitch += pitch & 1
    return pitch, pitch % 2 == 0


def kappa_loss(Psi, D, loss, weight, eps):
    """(P,): the Lipschitz factor of the residual pass, relative: with k(r) = |dG/dPsi| + |dG/dPsi*| per pixel (the norm of the
    real-linear map dPsi -> dG), kappa = rms_r(k) rms(Psi) / rms(G): a homogeneous error of e rms(Psi) on Psi leaves at most
    kappa e rms(G) on G.  With a = |Psi|, I = a^2 (Psi, D unshifted; D (P, nx, ny), weight (nx, ny) or None, both already unshifted):
        amplitude   dG/dPsi = w (1 - sqrt D / (2 a)),                       |dG/dPsi*| = w sqrt D / (2 a)
        intensity   dG/dPsi = w (2 I - D),                                  |dG/dPsi*| = w I
        poisson     dG/dPsi = w (1 - D / (I + eps) + D I / (I + eps)^2),    |dG/dPsi*| = w D I / (I + eps)^2"""
    a = np.abs(Psi)
    I = a * a
    w = 1.0 if weight is None else weight[None]
    if loss == "amplitude":
        r = np.sqrt(D) / (2.0 * np.maximum(a, np.sqrt(eps)))
        k, G = w * (np.abs(1.0 - r) + r), w * (1.0 - 2.0 * r) * a
    elif loss == "intensity":
        k, G = w * (np.abs(2.0 * I - D) + I), w * (I - D) * a
    else:
        r = D / (I + eps)
        k, G = w * (np.abs(1.0 - r + r * I / (I + eps)) + r * I / (I + eps)), w * (1.0 - r) * a
    ms = lambda v: (np.abs(v) ** 2).mean(axis=(1, 2))
    return np.sqrt(ms(k) * ms(a) / ms(G))


def white_loss_bound(Psi, D, L, loss, eps, e):
    """(P,): the algebra of tests/gradient_cases.py's loss_bound for exit amplitudes a = |Psi| that move by delta with
    ||delta||_2 <= e ||a||_2 (S = sum I; D unshifted):
        amplitude   2 e sqrt(L S) + e^2 S
        intensity   E = 2 e max(a) sqrt(S) + e^2 S;  sqrt(2 L0) E + E^2 / 2,  L0 the unweighted loss
        poisson     2 e sqrt(S) (sqrt(S) + ||D a / (I + eps)||_2) + e^2 S (1 + 6 max(D / (I + eps))),  which needs eps >= 4 e^2 S
    A weight 0 <= w <= 1 only takes terms out."""
    I = np.abs(Psi) ** 2
    S = I.sum(axis=(1, 2))
    L = np.abs(L)
    if loss == "amplitude":
        return 2.0 * e * np.sqrt(L * S) + e * e * S
    if loss == "intensity":
        E = 2.0 * e * np.sqrt(I.max(axis=(1, 2))) * np.sqrt(S) + e * e * S
        return np.sqrt(((I - D) ** 2).sum(axis=(1, 2))) * E + 0.5 * E * E
    assert (eps >= 4.0 * e * e * S).all()
    r = D / (I + eps)
    return 2.0 * e * np.sqrt(S) * (np.sqrt(S) + np.sqrt(((r * np.sqrt(I)) ** 2).sum(axis=(1, 2)))) + e * e * S * (1.0 + 6.0 * r.max(axis=(1, 2)))


def gradient_inputs(c):
    """the inputs of a case, nothing computed from them yet: V (nz, nx, ny) float32; the weight (nx, ny) float32 in the detector's
    layout -- uniform in [0, 1], about a quarter of the pixels exactly 0, not symmetric under i -> n - i -- or None; per add the
    (P, nx, ny) complex64 probes and the u (B, nx, ny) of its data"""
    seed = (c.nx * 4099 + c.ny) * 64 + c.nz * 8 + c.P
    probes, V = white_input(c.nx, c.ny, c.nz, c.P)
    rng = np.random.default_rng(seed + 977)
    w = None
    if c.weighted:
        w = rng.random((c.nx, c.ny)).astype(np.float32)
        w[rng.random((c.nx, c.ny)) < 0.25] = 0.0
    adds = []
    for a, B in enumerate(c.adds):
        pr = probes if a == 0 else white_input(c.nx, c.ny, c.nz, c.P, seed=seed + 31 * a)[0]
        adds.append((pr, rng.uniform(-1.0, 1.0, (B, c.nx, c.ny))))
    return V[0], w, adds


@functools.lru_cache(maxsize=4)
def gradient_data(c):
    """inputs, float64 reference (pyslice_amd/adjoint.py under the case's tilted propagator, on the float32 V widened) and bounds of
    a case; nothing of the device.  The data: sqrt D = |Psi_ref| (1 + U_RANGE u) in the detector's layout, rounded to float32 (what
    is uploaded and what the reference reads): G is then a white field for all three losses and sqrt D / |Psi| stays in
    [1 - U_RANGE, 1 + U_RANGE] at the Rayleigh field's near-zeros.  epsilon: 1e-20, for the Poisson loss 1e-6 of the first pattern's sum
    (gradient_cases.poisson_epsilon), as float32.

    Bounds, composed from the white-noise contract (tol = two_pass_tolerance per 2-D transform, in quadrature over the transforms, x
    LINE_FACTOR for a line, x PIXEL_FACTOR for a pixel):
        phi_s carries 2 s transforms:                    e_phi(s) = tol sqrt(max(2 s, 1))
        Psi carries n_f = 2 (nz - 1) + 1, the residual pass multiplies that error by kappa (kappa_loss, on the reference's own Psi and
        D), and g behind slice s carries 1 + 2 (nz - 1 - s) more:
                                                         e_g(s) = tol sqrt(kappa^2 n_f + 1 + 2 (nz - 1 - s))
        probe gradient (metrics()):                      e_g(0) x (1, LINE_FACTOR, PIXEL_FACTOR)
        accumulator, slice s, with m(f) = mean |f|^2, the sums over the adds a and their probes p, acc(r) the float32 sums of the step
        kernel (B products and B additions of an add, each within an ulp of sum_p |g_p| |phi_p|: (B + 4) ulp):
            image   2 sigma sqrt( sum (e_g^2 + e_phi^2 + e_g^2 e_phi^2) m(g_p) m(phi_p) ) + rms_r acc(r)
            line    LINE_FACTOR x the image bound
            pixel   2 sigma sum F e_g rms(g_p) |phi_p(r)| + F e_phi rms(phi_p) |g_p(r)| + F^2 e_g e_phi rms(g_p) rms(phi_p),  F = PIXEL_FACTOR,
                    + acc(r)
        all three figures are stated over the norm 2 sigma sqrt( sum m(g_p) m(phi_p) )
        loss per probe:                                  white_loss_bound at e = tol sqrt(n_f)"""
    from pyslice_amd import adjoint as adj
    from pyslice_amd.tilt import tilted_propagator
    nx, ny, nz = c.nx, c.ny, c.nz
    sigma = orc.interaction_sigma(EV)
    V32, w32, add_in = gradient_inputs(c)
    V = V32.astype(np.float64)
    prop = tilted_propagator(nx, ny, DX, DY, orc.wavelength(EV), DZ, tilt_object(c.tilt))
    w = None if w32 is None else w32.astype(np.float64)
    wu = None if w is None else np.fft.ifftshift(w)
    tol, n_f = two_pass_tolerance(nx, ny), 2 * (nz - 1) + 1
    e_phi = tol * np.sqrt(np.maximum(2.0 * np.arange(nz), 1.0))
    adds, eps = [], None
    for probes, u in add_in:
        B = len(u)
        psis, phis, Psi = adj.forward_waves(probes[:B], V, sigma, prop)
        D = (np.fft.fftshift(np.abs(Psi) * (1.0 + U_RANGE * u), axes=(-2, -1)) ** 2).astype(np.float32)
        if eps is None:
            eps = float(np.float32(1e-6 * float(D[0].astype(np.float64).sum()))) if c.loss == "poisson" else 1e-20
        L, G = adj.loss_and_residual(Psi, D, c.loss, w, eps)
        grad, pg, pairs = adj.backward(G, psis, V, sigma, prop)
        Du = np.fft.ifftshift(D.astype(np.float64), axes=(-2, -1))
        kappa = kappa_loss(Psi, Du, c.loss, wu, eps)
        e_g = tol * np.sqrt(kappa.max() ** 2 * n_f + 1.0 + 2.0 * (nz - 1 - np.arange(nz)))
        adds.append(dict(probes=probes, B=B, D=D, loss=L, grad=grad, probe=pg, pairs=pairs, kappa=kappa, e_g=e_g,
                         loss_bound=white_loss_bound(Psi, Du, L, c.loss, eps, tol * np.sqrt(n_f))))
    ms = lambda f: (np.abs(f) ** 2).mean(axis=(1, 2))
    norm, img, pix = np.zeros(nz), np.zeros(nz), np.zeros((nz, nx, ny))
    for s in range(nz):
        q = q_err = 0.0
        acc = np.zeros((nx, ny))
        for a in adds:
            g, phi = a["pairs"][s]
            mg, mp, eg, ep = ms(g), ms(phi), a["e_g"][s], e_phi[s]
            q += (mg * mp).sum()
            q_err += (eg * eg + ep * ep + eg * eg * ep * ep) * (mg * mp).sum()
            F = PIXEL_FACTOR
            pix[s] += 2.0 * sigma * (F * eg * np.sqrt(mg)[:, None, None] * np.abs(phi) + F * ep * np.sqrt(mp)[:, None, None] * np.abs(g)
                                     + F * F * eg * ep * np.sqrt(mg * mp)[:, None, None]).sum(axis=0)
            acc += 2.0 * sigma * (a["B"] + 4) * F32_ULP * (np.abs(g) * np.abs(phi)).sum(axis=0)
        norm[s] = 2.0 * sigma * np.sqrt(q)
        img[s] = 2.0 * sigma * np.sqrt(q_err) + np.sqrt((acc ** 2).mean())
        pix[s] += acc
    out = dict(V=V32, weight=w32, epsilon=eps, sigma=sigma, adds=adds, grad=sum(a["grad"] for a in adds), norm=norm, img_bound=img,
               pix_bound=pix, kappa=max(float(a["kappa"].max()) for a in adds))
    return out


def gradient_compare(c, data, acc, probe_grads, losses):
    """the accumulator (nz, nx, ny) and per add the probe gradient (B, nx, ny) and the losses (B,) of a run against gradient_data ->
    dict(slices=[(E_img, E_line, E_pix) over the norm], slices_of=[their ratios to the bounds], probe=[metrics() per add],
    probe_of=[ratios], loss_of=[per add, (B,) ratios], worst=the largest ratio)"""
    res = dict(slices=[], slices_of=[], probe=[], probe_of=[], loss_of=[])
    for s in range(c.nz):
        d = np.abs(np.asarray(acc[s], dtype=np.float64) - data["grad"][s])
        line = max(np.sqrt((d ** 2).mean(axis=0)).max(), np.sqrt((d ** 2).mean(axis=1)).max())
        rms = np.sqrt((d ** 2).mean())
        res["slices"].append((rms / data["norm"][s], line / data["norm"][s], d.max() / data["norm"][s]))
        res["slices_of"].append((rms / data["img_bound"][s], line / (LINE_FACTOR * data["img_bound"][s]), (d / data["pix_bound"][s]).max()))
    for a, pg, L in zip(data["adds"], probe_grads, losses):
        m = metrics(pg, a["probe"])
        res["probe"].append(m)
        res["probe_of"].append(tuple(v / (f * a["e_g"][0]) for v, f in zip(m, (1.0, LINE_FACTOR, PIXEL_FACTOR))))
        res["loss_of"].append(np.abs(np.asarray(L) - a["loss"]) / a["loss_bound"])
    res["worst"] = float(max([max(r) for r in res["slices_of"] + res["probe_of"]] + [r.max() for r in res["loss_of"]]))
    return res


def _gradient_run(eng, c, data):
    probe_grads, losses = [], []
    for a in data["adds"]:
        eng.upload_probes(a["probes"])
        L, pg = eng.adjoint_add(a["D"], B=a["B"], probe=True)
        losses.append(L)
        probe_grads.append(pg)
    return eng.adjoint_download(), probe_grads, losses


def gradient_case(c, restore=False):
    """one engine: upload_potential, set_tilt (a tilted case), set_adjoint, then per add upload_probes and adjoint_add, and
    adjoint_download -> gradient_compare's dict, with pitch and vec (adjoint_layout: the row pitch and whether the 16-byte step ran),
    kappa, and for a tilted case moved = (rel-L2 of the accumulator, of the first probe gradient) against the UNTILTED reference on the
    same data.  restore: then set_tilt(0, 0) and adjoint_reset on the same handle and the untilted case of the same grid ->
    restored = its dict"""
    from pyslice_amd.adjoint import LOSSES
    data = gradient_data(c)
    eng = engine(c.nx, c.ny, c.nz, c.P, fft_path=c.fft_path)
    try:
        eng.upload_probes(data["adds"][0]["probes"])
        eng.upload_potential(data["V"])
        if c.tilt is not None:
            eng.set_tilt(*c.tilt)
        eng.set_adjoint(LOSSES[c.loss], data["epsilon"], data["weight"])
        pitch, vec = eng.adjoint_layout()
        got = _gradient_run(eng, c, data)
        res = gradient_compare(c, data, *got)
        res.update(pitch=pitch, vec=vec, kappa=data["kappa"])
        if c.tilt is not None:
            res["moved"] = gradient_moved(c, data, got[0], got[1][0])
        if restore:
            flat = c._replace(tilt=None)
            fdata = gradient_data(flat)
            assert fdata["epsilon"] == data["epsilon"] or c.loss != "poisson"
            eng.set_tilt(0.0, 0.0)
            eng.adjoint_reset()
            res["restored"] = gradient_compare(flat, fdata, *_gradient_run(eng, flat, fdata))
    finally:
        eng.close()
    return res


def gradient_moved(c, data, acc, probe_grad):
    """(rel-L2 of an accumulator, of the first add's probe gradients) against the float64 definition WITHOUT the tilt on the case's
    own probes, potential, data and weight: what a tilt that never reached the backward loop -- or the forward one -- would give"""
    from pyslice_amd import adjoint as adj
    from pyslice_amd.tilt import tilted_propagator
    prop = tilted_propagator(c.nx, c.ny, DX, DY, orc.wavelength(EV), DZ, None)
    w = None if data["weight"] is None else data["weight"].astype(np.float64)
    grad, pg0 = 0.0, None
    for a in data["adds"]:
        g, _, pg = adj.potential_gradient(a["probes"][:a["B"]], data["V"].astype(np.float64), a["D"], data["sigma"], prop, c.loss, w, data["epsilon"])
        grad, pg0 = grad + g, pg if pg0 is None else pg0
    return _rel_l2(acc, grad), _rel_l2(probe_grad, pg0)


def gradient_main(out_path):
    """every GRAD_* case -> the figures and their ratios to the bounds, per case"""
    rows = ["White-spectrum parity of the slice loop backwards (tools/white_parity.py --gradient-only): white probes, white potentials, white",
            "data and weights through msl_adjoint_add against pyslice_amd/adjoint.py in float64.  Per case the worst figure over the slices",
            "of the accumulator (E_img, E_line, E_pix over 2 sigma sqrt(sum_p mean|g_p|^2 mean|phi_p|^2)), over the probe gradients",
            "(metrics()) and the largest ratio of each to its bound (gradient_data's docstring); loss: the largest |got - want| / bound.",
            "The bounds of tests/test_gpu_white_gradient.py are not taken from this file.", "",
            f"{'list':12s} {'case':44s} {'pitch':>5s} {'vec':>5s} {'kappa':>5s}   acc: E_img E_line E_pix   of bound: img line pix | probe of bound: img line pix | loss | moved"]
    bad = 0
    cases = [(name, c, False) for name, cases in GRADIENT_LISTS for c in cases] + [("restore", GRAD_RESTORE_CASE, True)]
    for name, c, restore in cases:
        res = gradient_case(c, restore=restore)
        for tag, r in ((gradient_id(c), res),) + ((("(0, 0) again", res["restored"]),) if restore else ()):
            sl, so = np.max(r["slices"], axis=0), np.max(r["slices_of"], axis=0)
            po, lo = np.max(r["probe_of"], axis=0), max(v.max() for v in r["loss_of"])
            bad += not r["worst"] <= 1.0
            moved = " ".join(f"{v:.2f}" for v in res["moved"]) if "moved" in res and r is res else "-"
            rows.append(f"{name:12s} {tag:44s} {res['pitch']:5d} {str(res['vec']):>5s} {res['kappa']:5.2f}   " + " ".join(f"{v:.2e}" for v in sl) + "   " +
                        " ".join(f"{v:.3f}" for v in so) + " | " + " ".join(f"{v:.3f}" for v in po) + f" | {lo:.3f} | {moved}" + ("" if r["worst"] <= 1.0 else " <-- ABOVE"))
            print(rows[-1], flush=True)
    rows += ["", f"{len(cases)} cases, {bad} results above a bound"]
    text = "\n".join(rows) + "\n"
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    if "--gradient-only" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--gradient-only"]
        sys.exit(gradient_main(args[0] if args else None))
    if "--output-only" in sys.argv[1:]:
        args = [a for a in sys.argv[1:] if a != "--output-only"]
        sys.exit(output_main(args[0] if args else None))
    args = [a for a in sys.argv[1:] if a != "--tilt-only"]
    if "--tilt-only" in sys.argv[1:]:
        sys.exit(tilt_main(args[0] if args else None))
    rc = main(args[0] if args else None)
    sys.exit(tilt_main(args[1] if len(args) > 1 else None) or rc)

"""White-spectrum parity of the slice-loop passes through the C ABI: white-noise probes through unit-modulus random phase screens
(the Fresnel factor is unit modulus too, so the waves stay white in both spaces through every slice), against the float64 oracle,
per image, per line and per pixel.  tests/test_gpu_white_spectrum.py imports white_case(), the case lists and the bounds; run as
a script it measures every case, on the one-pass kernels and on the generic two-pass loop (fft_path=1), and writes the worst
figures per kernel family.

With tilt=(tan_x, tan_y) the same cases run on the tables msl_set_tilt writes, which are not even in k (P[m] != P[n - m]), against
the float64 definition of pyslice_amd/tilt.py: tests/test_gpu_white_tilt.py imports the TILT_* lists, and the script measures them
into a second report.  usage: python tools/white_parity.py [out.txt [tilt_out.txt]], or --tilt-only [tilt_out.txt]"""
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


def engine(nx, ny, nz, P, n_frames=1, fft_path=0, frame_batch=1):
    return _native.Engine(nx, ny, nz, DX, DY, DZ, orc.wavelength(EV), orc.interaction_sigma(EV), n_probes=P, n_frames=n_frames,
                          fft_path=fft_path, frame_batch=frame_batch)


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


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tilt-only"]
    if "--tilt-only" in sys.argv[1:]:
        sys.exit(tilt_main(args[0] if args else None))
    rc = main(args[0] if args else None)
    sys.exit(tilt_main(args[1] if len(args) > 1 else None) or rc)

"""White-spectrum parity of the potential build through the C ABI: flat ("white") form factors, so that every k-bin of the structure
factor R_s carries the same weight, against a float64 restatement of the oracle's formula, per image, per k-bin, per k-line and per
pixel.  With the physical Kirkland table max|dV| / max|V| is blind to a wrong bin at high k (f_Z falls off steeply and max|V| is the
peak at an atom); with a flat table a bin that is 50 % wrong is 0.5 of the rms of its line.
tests/test_white_potential_host.py and tests/test_gpu_white_potential.py import the table, the reference, the metrics, the bounds,
path() and the case lists; run as a script it measures every case and writes the worst figures per kernel family.
usage: python tools/white_potential.py [out.txt]"""
import collections
import functools
import os
import sys
import numpy as np
_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, ".."))
sys.path.insert(0, _HERE)
from oracle import multislice_oracle as orc
from pyslice_amd import _native
import white_parity as wpar

EV = 100e3
DX, DY, DZ = 0.1, 0.09, 0.5            # dx != dy: a form-factor table indexed with the axes swapped shows on the Gaussian species
WHITE_CONSTS = {5: 1.0, 7: -0.7, 14: 0.45}     # B, N, Si: different in sign and size, so that a species mix-up shows
GAUSS_Z = 14                           # this species gets c exp(-d q^2), a factor 2 down at the corner of k-space
SPECIES = (5, 7, 14)
RMS_PHASE = 0.3                        # rms of sigma V: complex64 rounding of t is then about 2e-7 of the rms of V
TOL_DIRECT, TOL_CONV = wpar.TOL_DIRECT, wpar.TOL_CONV             # per 2-D transform (test_fft2_matches_numpy)
LINE_FACTOR, PIXEL_FACTOR = wpar.LINE_FACTOR, wpar.PIXEL_FACTOR   # a k-line is a smaller sample; the largest of ~1e5 errors
MOD_BOUND = 4.0 * 2.0 ** -24           # | |t| - 1 |
EMPTY_BOUND = 2.0 ** -23               # | t - 1 | of a slice without atoms
METRICS = ("E_img", "E_kline", "E_bin", "E_pix", "E_mod")

Case = collections.namedtuple("Case", "nx ny nz density keep fft_path env batch kind slice_axis", defaults=(False, 0, (), 1, "uniform", 2))
NO_TWO_LINE, NO_PAIRED = ("MSL_NO_TWO_LINE_IFFT",), ("MSL_NO_PAIRED_IFFT",)

# ---- case lists (tests/test_gpu_white_potential.py runs exactly these) ------------------------------------------------------------
# structure-factor kernels x edge handling: 256 x 256 x 2 keeps the inverse transform the same four-step pass
SF_CASES = [Case(256, 256, 2, "sparse"), Case(256, 256, 2, "dense"), Case(256, 256, 2, "dense", env=("MSL_SF_F32",)),
            Case(256, 256, 2, "dense", env=("MSL_SF_TWO_TILES",)), Case(96, 80, 2, "dense", env=("MSL_SF_TWO_TILES",)),
            Case(320, 200, 2, "dense", env=("MSL_SF_TWO_TILES",)), Case(2048, 2048, 2, "dense")]
# the edge kernel serves n even with (n/2 + 1) % 32 == 1: on x only, on y only, on both (the corner bin), on neither, odd lengths
EDGE_CASES = [Case(nx, ny, 2, d) for nx, ny in ((256, 80), (80, 256), (64, 64), (128, 192), (96, 80), (45, 63)) for d in ("sparse", "dense")]
ROWS_CASES = [Case(96, 80, 2, "sparse", keep=True), Case(256, 256, 2, "sparse", fft_path=1)]
# inverse-transform forms, sparse; nz = 3 and nz = 2 store different slices transposed and leave the loop on different axes
LINES_CASES = [Case(nx, ny, nz, "sparse") for nx, ny in ((256, 256), (1024, 256)) for nz in (3, 2)] + \
              [Case(256, 256, 3, "sparse", keep=True), Case(256, 80, 3, "sparse"), Case(30, 28, 3, "sparse"), Case(45, 63, 3, "sparse"),
               Case(67, 37, 3, "sparse", keep=True), Case(1100, 48, 3, "sparse")]
CHIRPZ16_CASES = [Case(nx, ny, 3, "sparse") for nx, ny in ((33, 37), (128, 100), (127, 64))]
CHIRPZ32_CASES = [Case(nx, ny, nz, "sparse") for nx, ny in ((129, 191), (501, 491), (512, 300), (300, 135)) for nz in (3, 2)]
CHIRPZ32_SWITCH_CASES = [Case(501, 491, 3, "sparse", env=NO_TWO_LINE), Case(501, 491, 3, "sparse", env=NO_PAIRED)]
CHIRPZ64_CASES = [Case(nx, ny, 3, "sparse") for nx, ny in ((513, 135), (600, 135), (997, 37), (349, 1024), (1024, 37))]
TWO_CASES = [Case(512, 512, 3, "sparse"), Case(512, 512, 2, "sparse"), Case(512, 512, 3, "sparse", env=NO_PAIRED)]
WAVE2K_CASES = [Case(2048, 2048, 3, "sparse")]             # (the dense 2048 x 2048 x 2 case is in SF_CASES)
BATCH_CASES = [Case(nx, ny, 3, "sparse", batch=b) for nx, ny in ((256, 256), (501, 37), (512, 512)) for b in (2, 3)]
ATOM_KINDS = ("empty_middle", "single_species", "delta", "x0", "xL", "outside_box", "outside_slices", "axis0", "axis1")
ATOM_CASES = [Case(nx, ny, 3, "sparse", kind=k, slice_axis={"axis0": 0, "axis1": 1}.get(k, 2)) for nx, ny in ((256, 80), (501, 37)) for k in ATOM_KINDS]
SINGLE_CASES = list(dict.fromkeys(SF_CASES + EDGE_CASES + ROWS_CASES + LINES_CASES + CHIRPZ16_CASES + CHIRPZ32_CASES + CHIRPZ32_SWITCH_CASES +
                                 CHIRPZ64_CASES + TWO_CASES + WAVE2K_CASES + ATOM_CASES))       # (256 x 256 x 2 sparse is in two lists)
FLOOR_GRIDS = [(96, 80), (256, 256), (512, 300), (1024, 1024)]


# ---- the white table and the float64 reference --------------------------------------------------------------------------------------
def white_table(consts=None, dx=DX, dy=DY):
    """(103, 3, 4) float64 table (a, b, c, d) with a_i = 0, b_i = 1, c = (c_Z, 0, 0), d = 0: f_Z(q^2) = c_Z at every k; the species
    GAUSS_Z gets d = ln 2 / q_corner^2 instead, q_corner^2 = (1 / 2dx)^2 + (1 / 2dy)^2.  Species not in consts get f = 0."""
    t = np.zeros((103, 3, 4), dtype=np.float64)
    t[:, :, 1] = 1.0
    for Z, c in (WHITE_CONSTS if consts is None else consts).items():
        t[Z - 1, 0, 2] = c
        if Z == GAUSS_Z:
            t[Z - 1, 0, 3] = np.log(2.0) / ((0.5 / dx) ** 2 + (0.5 / dy) ** 2)
    return t


def form_factor(qsq, row):
    """f(q^2) = sum_i a_i / (q^2 + b_i) + sum_i c_i exp(-d_i q^2) for one (3, 4) row of a table"""
    out = np.zeros_like(qsq, dtype=np.float64)
    for a, b, c, d in row:
        out = out + a / (qsq + b)
    acc = np.zeros_like(qsq, dtype=np.float64)
    for a, b, c, d in row:
        acc = acc + c * np.exp(-d * qsq)
    return out + acc


def slice_edges(nz, dz):
    """[lo, hi) of the slices at 0, dz, 2 dz ...: slice 0 starts at 0, the last one ends at its coordinate + dz, inner edges half way"""
    lo = np.array([s * dz - dz / 2 if s > 0 else 0.0 for s in range(nz)], dtype=np.float64)
    hi = np.array([s * dz + dz / 2 if s < nz - 1 else (nz - 1) * dz + dz for s in range(nz)], dtype=np.float64)
    return lo, hi


def reference(nx, ny, nz, dx, dy, dz, pos, Z, table, slice_axis=2):
    """float64 structure factors R (nz, nx, ny) complex and potentials V (nz, nx, ny) of the formula of oracle.potential with the
    table as an argument:  R_s = sum_Z f_Z(q^2) sum_{a in Z, slice s} exp(-2 pi i (kx x_a + ky y_a)),  V_s = Re ifft2(R_s) / (dx^2 dy^2);
    the in-plane coordinates are the two axes left by slice_axis, in order"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    Z = np.asarray(Z)
    axes = [0, 1, 2]
    axes.remove(slice_axis)
    lo, hi = slice_edges(nz, dz)
    kxs, kys = np.fft.fftfreq(nx, d=dx), np.fft.fftfreq(ny, d=dy)
    qsq = kxs[:, None] ** 2 + kys[None, :] ** 2
    R = np.zeros((nz, nx, ny), dtype=np.complex128)
    for Zv in np.unique(Z):
        sel = pos[Z == Zv]
        fz = form_factor(qsq, table[int(Zv) - 1])
        zc = sel[:, slice_axis]
        for s in range(nz):
            m = (zc >= lo[s]) & (zc < hi[s])
            if not m.any():
                continue
            ex = np.exp(-2j * np.pi * np.outer(kxs, sel[m, axes[0]]))
            ey = np.exp(-2j * np.pi * np.outer(sel[m, axes[1]], kys))
            R[s] += (ex @ ey) * fz
    return R, potential_of(R, dx, dy)


def potential_of(R, dx=DX, dy=DY):
    return np.fft.ifft2(R, axes=(-2, -1)).real / (dx ** 2 * dy ** 2)


# ---- metrics and bounds ---------------------------------------------------------------------------------------------------------------
def _slice_metrics(dV, Vw, Rw, dx, dy):
    """(E_img, E_kline, E_bin, E_pix) of one slice and where the bin and the line are"""
    D2 = np.abs(np.fft.fft2(dV) * (dx ** 2 * dy ** 2)) ** 2
    R2 = np.abs(Rw) ** 2
    rows, cols = np.sqrt(D2.sum(axis=1) / R2.sum(axis=1)), np.sqrt(D2.sum(axis=0) / R2.sum(axis=0))
    line = ("kx", int(rows.argmax())) if rows.max() >= cols.max() else ("ky", int(cols.argmax()))
    e = (np.sqrt((dV ** 2).sum() / (Vw ** 2).sum()), max(rows.max(), cols.max()), np.sqrt(D2.max() / R2.mean()),
         np.abs(dV).max() / np.sqrt((Vw ** 2).mean()))
    return e, tuple(int(i) for i in np.unravel_index(D2.argmax(), D2.shape)), line


def _worst(per_slice, e_mod, e_empty):
    out = {"E_mod": float(e_mod), "E_empty": float(e_empty), "bin": None, "line": None}
    for i, name in enumerate(METRICS[:4]):
        out[name] = float(max((e[0][i] for e in per_slice), default=0.0))
    if per_slice:
        s = int(np.argmax([e[0][2] for e in per_slice]))
        out["bin"] = (per_slice[s][3],) + per_slice[s][1]
        s = int(np.argmax([e[0][1] for e in per_slice]))
        out["line"] = (per_slice[s][3],) + per_slice[s][2]
    return out


def metrics(t_got, V_want, R_want, sigma, dx=DX, dy=DY):
    """worst over the slices of a stack of transmission functions t_got (nz, nx, ny) against t_want = exp(i sigma V_want) in float64,
    through dV = Im(t_got conj t_want) / sigma (first order in the error, no phase wrap) and D = fft2(dV) dx^2 dy^2:
        E_img = |dV| / |V_want|                       E_pix = max |dV| / rms V_want
        E_bin = max_k |D_k| / rms_k |R_want|          E_kline = largest |D| / |R_want| over single k-rows and k-columns
        E_mod = max | |t_got| - 1 |
    A slice without atoms (R_want = 0) is left out of the ratios; E_empty = its max |t_got - 1|.  'bin' = (slice, kx, ky) of E_bin,
    'line' = (slice, 'kx' | 'ky', index) of E_kline."""
    t_got = np.asarray(t_got).astype(np.complex128)
    per_slice, e_mod, e_empty = [], 0.0, 0.0
    for s in range(t_got.shape[0]):
        e_mod = max(e_mod, np.abs(np.abs(t_got[s]) - 1.0).max())
        if not R_want[s].any():
            e_empty = max(e_empty, np.abs(t_got[s] - 1.0).max())
            continue
        dV = (t_got[s] * np.exp(-1j * sigma * V_want[s])).imag / sigma
        per_slice.append(_slice_metrics(dV, V_want[s], R_want[s], dx, dy) + (s,))
    return _worst(per_slice, e_mod, e_empty)


def metrics_potential(V_got, V_want, R_want, dx=DX, dy=DY):
    """the same figures on a kept potential V_got (nz, nx, ny) float32 itself: dV = V_got - V_want (E_mod = 0; E_empty = max |V_got|)"""
    V_got = np.asarray(V_got).astype(np.float64)
    per_slice, e_empty = [], 0.0
    for s in range(V_got.shape[0]):
        if not R_want[s].any():
            e_empty = max(e_empty, np.abs(V_got[s]).max())
            continue
        per_slice.append(_slice_metrics(V_got[s] - V_want[s], V_want[s], R_want[s], dx, dy) + (s,))
    return _worst(per_slice, 0.0, e_empty)


def contrast_distance(t_got, V_want, sigma):
    """|t_got - t_want| / |t_want - 1|: about sqrt 2 for the stack of another frame.  (Not E_img: dV = sin(sigma (V - V_want)) / sigma
    saturates at the atoms of a spiky potential, where sigma V is many radians and most of |V| sits -- the float64 reference of one
    frame against that of another gives E_img 0.45 .. 0.76 on the batch cases.)"""
    t_want = np.exp(1j * sigma * V_want)
    return float(np.linalg.norm(np.asarray(t_got).astype(np.complex128) - t_want) / np.linalg.norm(t_want - 1.0))


def bounds(tol, peak_phase):
    """the bounds of a case from the tolerance of its inverse transform: the white-noise contract per 2-D transform, the line and
    extreme-value factors of tools/white_parity.py; peak_phase = max |sigma V_want| of the case: fp32 rounding of sigma V at a peak
    pixel of a spiky potential (few atoms: peak / rms ~ sqrt(N / n_atoms)) adds 2^-24 peak_phase / RMS_PHASE to E_pix alone"""
    return {"E_img": tol, "E_kline": LINE_FACTOR * tol, "E_bin": PIXEL_FACTOR * tol,
            "E_pix": PIXEL_FACTOR * tol + 2.0 ** -24 * peak_phase / RMS_PHASE, "E_mod": MOD_BOUND, "E_empty": EMPTY_BOUND}


def excess(m, b):
    """largest ratio of a figure to its bound, and its name"""
    return max((m[k] / b[k], k) for k in METRICS + ("E_empty",))


# ---- what the library runs on a grid (mslice.hip: msl_create, plan_axis_kind, make_axis_tables, plan_pot_ifft, launch_structure_factor) -----
def _plan_M(n):
    """length of the generic plan: n where it factors into 8 4 2 3 5 7 11 13 (at most 16 stages), else the power of two >= 2n - 1"""
    m, stages = n, 0
    for r in (8, 4, 2, 3, 5, 7, 11, 13):
        while m % r == 0 and m > 1:
            m //= r
            stages += 1
    if m == 1 and stages <= 16:
        return n
    M = 1
    while M < 2 * n - 1:
        M <<= 1
    return M


def _axis_base(n, n_other, rfast, want):
    lines_ok = n_other % 16 == 0
    if not want:
        return "none"
    if rfast and lines_ok:
        return "four-step"
    if n in (512, 2048) and lines_ok:
        return "2R^2" if n == 512 else "wave-2K"
    if 33 <= n <= 512 and (n <= 128 or n >= 192 or _plan_M(n) != n):
        return "conv"
    if 513 <= n <= 1024:
        return "conv2k"
    if 1025 <= n <= 2047:
        return "conv4k"
    return "generic" if _plan_M(n) <= 1024 else "none"


Path = collections.namedtuple("Path", "form ifft sf one_pass half_rows tol label")


def path(nx, ny, keep_potential=False, fft_path=0, atoms_per_bin=0.0, env=()):
    """the kernels the potential build runs: form (PI_LINES / PI_TWO / PI_CHIRPZ / PI_WAVE2K), the inverse transform per axis
    (y first), the structure-factor kernel with its edge kernel, whether the slice loop is one-pass, whether half rows are written,
    the tolerance of the inverse transform, and a label for test ids.  atoms_per_bin = atoms / (slices x species); env = the debug
    switches set (with MSL_DEBUG)."""
    fr = lambda n: 32 if n == 1024 else 16 if n == 256 else 0
    ry = fr(ny) if fft_path == 0 and fr(ny) and nx % (256 // fr(ny)) == 0 else 0
    rx = fr(nx) if fft_path == 0 and ny % 16 == 0 and ny >= 32 else 0
    bx, by = _axis_base(nx, ny, rx, fft_path == 0), _axis_base(ny, nx, ry, fft_path == 0)
    one_pass = bx != "none" and by != "none"
    conv = lambda b: b in ("conv", "conv2k")
    cz = lambda n, b, other: (16 if n <= 128 else 32 if n <= 512 else 64) if conv(b) or (conv(other) and 33 <= n <= 1024) else 0
    czx, czy = cz(nx, bx, by), cz(ny, by, bx)
    generic = lambda n: "generic" if _plan_M(n) == n else "bluestein"
    if not one_pass or keep_potential:
        form = "PI_LINES"
    elif bx == "wave-2K" and by == "wave-2K":
        form = "PI_WAVE2K"
    elif czx and czy:
        form = "PI_CHIRPZ"
    elif bx == "2R^2" and by == "2R^2":
        form = "PI_TWO"
    else:
        form = "PI_LINES"
    if form == "PI_LINES":
        ifft = ("four-step" if ry else generic(ny), "four-step" if rx else generic(nx))
        half_rows = bool(rx and ry)
        if half_rows:
            ifft = ("four-step", "four-step-herm")
    elif form == "PI_CHIRPZ":
        second = {16: "ifftTB16", 32: "ifftTB32" if "MSL_NO_PAIRED_IFFT" in env else "ifftTB32pair", 64: "ifftTB2"}[czx]
        first = {16: "ifftTB16", 32: "ifftTB32" if "MSL_NO_TWO_LINE_IFFT" in env else "ifftTB_two", 64: "ifftTB2"}[czy]
        ifft, half_rows = (first, second), True
    elif form == "PI_TWO":
        ifft, half_rows = ("ifftT2", "ifftT2" if "MSL_NO_PAIRED_IFFT" in env else "ifftT2pair"), True      # 512 lines: a multiple of 32
    else:
        ifft, half_rows = ("ifftTW", "ifftTW"), True
    tol = TOL_CONV if form == "PI_CHIRPZ" or "bluestein" in ifft else TOL_DIRECT
    cx, cy = nx // 2 + 1, ny // 2 + 1
    edge_x, edge_y = nx % 2 == 0 and cx % 32 == 1 and cx > 1, ny % 2 == 0 and cy % 32 == 1 and cy > 1
    tiles_x, tiles_y = (cx // 32 if edge_x else (cx + 31) // 32), (cy // 32 if edge_y else (cy + 31) // 32)
    if atoms_per_bin >= 128.0 and "MSL_SF_TILED" not in env:
        if "MSL_SF_F32" in env:
            sf = "stream"
        elif (tiles_x * tiles_y >= 512 or (tiles_x >= 2 and "MSL_SF_TWO_TILES" in env)) and "MSL_SF_ONE_TILE" not in env:
            sf = "bf16x2"
        else:
            sf = "stream_bf16"
    else:
        sf = "quad"
    sf += {(0, 0): "", (1, 0): "+edge_x", (0, 1): "+edge_y", (1, 1): "+edge_xy"}[(int(edge_x), int(edge_y))]
    label = f"{form[3:]}.{ifft[0]}.{ifft[1]}-{sf}"
    return Path(form, ifft, sf, one_pass, half_rows, tol, label)


def case_path(c):
    return path(c.nx, c.ny, c.keep, c.fft_path, atoms_per_bin(c), c.env)


def case_id(c):
    extra = "".join(f"-{v}" for v in (("keep" if c.keep else ""), (f"fft_path{c.fft_path}" if c.fft_path else ""), (f"batch{c.batch}" if c.batch > 1 else ""),
                                      ("" if c.kind == "uniform" else c.kind)) + tuple(e[4:].lower() for e in c.env) if v)
    return f"{c.nx}x{c.ny}x{c.nz}-{c.density}{extra}-{case_path(c).label}"


# ---- atoms ------------------------------------------------------------------------------------------------------------------------------
def bin_counts(c, frame=0):
    """atoms per (slice, species) of a case: sparse 20 .. 60 (the tiled kernel), dense 130 .. 200 (the streaming kernels), bin sizes
    that are and are not multiples of 16"""
    rng = np.random.default_rng((c.nx * 4099 + c.ny) * 64 + c.nz * 8 + frame)
    lo, hi = (20, 60) if c.density == "sparse" else (130, 200)
    n = rng.integers(lo, hi + 1, size=(c.nz, len(SPECIES)))
    n[0, 0] = 48 if c.density == "sparse" else 144                  # a multiple of 16 ...
    n[-1, -1] = 37 if c.density == "sparse" else 197                # ... and a bin that is none
    if c.kind == "empty_middle":
        n[c.nz // 2] = 0
    if c.kind == "single_species":
        n[c.nz // 2, 1:] = 0
    if c.kind == "delta":
        n[c.nz // 2] = 0                 # the one atom of this slice is added by atoms()
    return n


def atoms_per_bin(c):
    """atoms / (slices x species) as launch_structure_factor counts them (every atom handed over, in a slice or not)"""
    extra = {"delta": 1, "outside_slices": 12}.get(c.kind, 0)
    return (int(bin_counts(c).sum()) + extra) / (c.nz * len(SPECIES))


def atoms(c, frame=0):
    """positions (n, 3) and Z (n,) of a case: uniform random in the box, every slice's atoms inside its [lo, hi); the same Z in
    every frame of a batch (frames differ in the positions)"""
    n = bin_counts(c)                   # the same counts in every frame: one Z array per batch
    rng = np.random.default_rng((c.nx * 4099 + c.ny) * 64 + c.nz * 8 + 1000 + frame)
    lo, hi = slice_edges(c.nz, DZ)
    lx, ly = c.nx * DX, c.ny * DY
    pos, Z = [], []
    for s in range(c.nz):
        for j, Zv in enumerate(SPECIES):
            k = int(n[s, j])
            p = np.empty((k, 3))
            p[:, 0], p[:, 1] = rng.random(k) * lx, rng.random(k) * ly
            p[:, 2] = lo[s] + (0.02 + 0.96 * rng.random(k)) * (hi[s] - lo[s])
            pos.append(p)
            Z.append(np.full(k, Zv, dtype=np.int32))
    pos, Z = np.concatenate(pos), np.concatenate(Z)
    pick = lambda k: rng.choice(len(pos), size=k, replace=False)
    if c.kind == "delta":                                   # a single atom exactly on a grid point: V is a delta, |R| = |c_Z| in every bin
        mid = c.nz // 2
        pos = np.concatenate([pos, [[(c.nx // 3) * DX, (c.ny // 5) * DY, 0.5 * (lo[mid] + hi[mid])]]])
        Z = np.concatenate([Z, np.array([7], dtype=np.int32)])
    elif c.kind == "x0":
        i = pick(12); pos[i[:6], 0] = 0.0; pos[i[4:], 1] = 0.0
    elif c.kind == "xL":
        i = pick(12); pos[i[:6], 0] = lx - 1e-9; pos[i[4:], 1] = ly - 1e-9
    elif c.kind == "outside_box":                           # the reference's phases are periodic
        i = pick(16); pos[i[:4], 0] = -0.37 * lx; pos[i[4:8], 0] = 1.6 * lx; pos[i[8:12], 1] = -0.37 * ly; pos[i[12:], 1] = 1.6 * ly
    elif c.kind == "outside_slices":                        # below the first and above the last slice: in no bin
        extra = np.column_stack([rng.random(12) * lx, rng.random(12) * ly, np.where(np.arange(12) < 6, -0.3, hi[-1] + 0.2)])
        pos = np.concatenate([pos, extra])
        Z = np.concatenate([Z, np.array([5, 7, 14] * 4, dtype=np.int32)])
    if c.slice_axis != 2:                                   # (x, y, z) -> the slice coordinate on slice_axis, in-plane axes in order
        axes = [0, 1, 2]
        axes.remove(c.slice_axis)
        q = np.empty_like(pos)
        q[:, axes[0]], q[:, axes[1]], q[:, c.slice_axis] = pos[:, 0], pos[:, 1], pos[:, 2]
        pos = q
    return pos, Z


@functools.lru_cache(maxsize=2)
def case_reference(nx, ny, nz, density, batch, kind, slice_axis):
    """(positions per frame, Z, R per frame, V per frame, sigma) of a case, computed once for the runs that share it (the debug
    switches, keep_potential and fft_path do not change the input)"""
    c = Case(nx, ny, nz, density, batch=batch, kind=kind, slice_axis=slice_axis)
    table = white_table()
    frames = [atoms(c, f) for f in range(batch)]
    Z = frames[0][1]
    RV = [reference(nx, ny, nz, DX, DY, DZ, p, Z, table, slice_axis) for p, _ in frames]
    full = [V[s] for R, V in RV for s in range(nz) if R[s].any()]
    sigma = RMS_PHASE / np.sqrt(np.mean(np.square(full)))
    return [p for p, _ in frames], Z, [r for r, _ in RV], [v for _, v in RV], float(sigma)


def white_potential_case(c):
    """build the potential(s) of a case on the device (the debug switches of c.env must be in the environment, with MSL_DEBUG) ->
    dict(t=[metrics per batch slot], V=metrics of potential() with keep_potential, bounds, raw=[t per slot], one_pass,
    cross=contrast_distance of slot 0 from the reference of slot 1)"""
    pos, Z, R, V, sigma = case_reference(c.nx, c.ny, c.nz, c.density, c.batch, c.kind, c.slice_axis)
    eng = _native.Engine(c.nx, c.ny, c.nz, DX, DY, DZ, orc.wavelength(EV), sigma, n_probes=1, n_frames=c.batch if c.batch > 1 else 0,
                         keep_potential=c.keep, fft_path=c.fft_path, frame_batch=c.batch)
    assert eng.frame_batch == c.batch
    eng.set_kirkland(white_table())
    eng.set_slices(*orc.slice_edges(np.arange(c.nz) * DZ))
    if c.batch > 1:
        eng.build_potentials(np.stack(pos), Z, c.slice_axis)
    else:
        eng.build_potential(pos[0], Z, c.slice_axis)
    raw = []
    for b in range(c.batch):
        if c.batch > 1:
            eng.select_batch_slot(b)
        raw.append(np.asarray(eng.transmission()))
    out = {"t": [metrics(raw[b], V[b], R[b], sigma) for b in range(c.batch)], "raw": raw, "V": None, "cross": None}
    if c.keep:
        out["V"] = metrics_potential(eng.potential(), V[0], R[0])
    if c.batch > 1:
        out["cross"] = contrast_distance(raw[0], V[1], sigma)
    # the slice loop on this engine: 16 bytes per pixel and slice-step on the one-pass loop, 32 on the two-pass loop
    eng.upload_probes(np.ones((1, c.nx, c.ny), dtype=np.complex64))
    eng.reset_counters()
    eng.propagate()
    out["one_pass"] = eng.counters()["algorithmic_bytes"] == (16 + 8) * c.nz * c.nx * c.ny
    eng.close()
    out["bounds"] = bounds(case_path(c).tol, sigma * max(np.abs(v).max() for v in V))
    return out


# ---- script mode -----------------------------------------------------------------------------------------------------------------------
def main(out_path):
    worst, bad, n_cases = {}, 0, 0
    for c in SINGLE_CASES + BATCH_CASES:
        saved = {k: os.environ.get(k) for k in ("MSL_DEBUG",) + c.env}
        if c.env:
            os.environ.update({k: "1" for k in ("MSL_DEBUG",) + c.env})
        try:
            res = white_potential_case(c)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        p, b = case_path(c), res["bounds"]
        runs = res["t"] + ([res["V"]] if res["V"] else [])
        over = max(excess(m, b) for m in runs)
        bad += over[0] > 1.0
        n_cases += 1
        m = max(runs, key=lambda r: excess(r, b))
        print(f"{case_id(c):90s} " + " ".join(f"{k[2:]} {m[k]:.2e}" for k in METRICS) + f" | of bound {over[0]:.2f} ({over[1]})"
              + (f" bin {m['bin']} line {m['line']}" if over[0] > 1.0 else "") + ("" if res["one_pass"] == p.one_pass else "   one_pass differs from path()"), flush=True)
        for fam in (f"{p.form[3:]} {p.ifft[0]} / {p.ifft[1]}", f"sf {p.sf}"):
            w = worst.setdefault(fam, {"n": 0, **{k: 0.0 for k in METRICS}, **{"r" + k: 0.0 for k in METRICS}})
            w["n"] += 1
            for r in runs:
                for k in METRICS:
                    w[k], w["r" + k] = max(w[k], r[k]), max(w["r" + k], r[k] / b[k])
    rows = ["White-spectrum parity of the potential build (tools/white_potential.py): flat form factors (B, N, Si = 1, -0.7, 0.45; Si with",
            "c exp(-d q^2), a factor 2 down at the corner of k-space), dx = 0.1, dy = 0.09, sigma = 0.3 / rms V, transmission functions (and kept",
            "potentials) against the float64 formula.  Worst figure of every case of a kernel family: a case counts once for its inverse-transform",
            "form (y pass / x pass) and once for its structure-factor kernel.  img: rel-L2 of dV; kline: largest rel-L2 of D = fft2(dV) over single",
            "k-rows and k-columns; bin: max |D_k| / rms |R|; pix: max |dV| / rms V; mod: max ||t| - 1|.  'of bound': the largest ratio to the bound",
            "of the case, tol x (1, 2, 10, 10 + the peak-rounding term) with tol = 3e-6 (direct axes) or 1e-5 (chirp-z or Bluestein axis), 4 x 2^-24",
            "for mod.  The bounds of tests/test_gpu_white_potential.py are not taken from this file.", "",
            f"{'family':44s} {'cases':>5s} " + " ".join(f"{k[2:]:>9s}" for k in METRICS) + "   of bound: " + " ".join(f"{k[2:]:>5s}" for k in METRICS)]
    for fam, w in sorted(worst.items()):
        rows.append(f"{fam:44s} {w['n']:5d} " + " ".join(f"{w[k]:9.2e}" for k in METRICS) + "             " + " ".join(f"{w['r' + k]:5.2f}" for k in METRICS))
    rows += ["", f"{n_cases} cases, {bad} above a bound"]
    text = "\n".join(rows) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else None))

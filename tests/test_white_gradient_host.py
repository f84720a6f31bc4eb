"""Host checks of gradient_case(), its bounds and the GRAD_* lists of tools/white_parity.py, the yardstick of
tests/test_gpu_white_gradient.py: no device needed.

- kappa_loss <= KAPPA_CAP for every listed case, the weight is white, a quarter zero and not symmetric, and the lists reach both step
  variants, every loss, the ragged add and P = 1;
- a complex64 / float32 evaluation of the loop of msl_adjoint_add (torch FFTs, the float32 sums of the step kernel, the float64
  accumulator) on exactly the device lists' inputs stays inside a third of every bound: the margin the bounds are judged against;
- each fault of FAULTS, built into that model, exceeds a bound by the factor stated there; next to it, whether the aggregate bounds of
  tests/gradient_cases.py on the physical inputs of test_gpu_gradient.py (101 x 97 x 4, three probes at probe_batch=2) see it;
- the call order of gradient_case on a float64 engine, and that a tilt which never reaches it is seen."""
import importlib.util
import os

import numpy as np
import pytest

import gradient_cases as gc

_spec = importlib.util.spec_from_file_location("white_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "white_parity.py"))
wp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wp)
orc = wp.orc

ALL_CASES = [c for _, cases in wp.GRADIENT_LISTS for c in cases]
AX = (-2, -1)


# ---- the lists ---------------------------------------------------------------------------------------------------------------------
def test_the_lists_reach_both_step_variants_every_loss_and_both_batch_forms():
    layouts = {(c.nx, c.ny, c.fft_path): wp.step_layout(c.nx, c.ny, c.fft_path) for c in ALL_CASES}
    assert layouts[(45, 63, 1)] == (63, False) and layouts[(101, 97, 0)] == (114, True) and layouts[(24, 20, 0)] == (36, True)
    assert layouts[(256, 64, 0)][1] and layouts[(12, 1050, 0)] == (1066, True)
    assert {v[1] for v in layouts.values()} == {True, False}
    for grid in ((45, 63), (101, 97)):
        assert {c.loss for c in ALL_CASES if (c.nx, c.ny) == grid} == set(wp.GRAD_LOSSES)
        assert any(c.adds == (3, 2) and c.P == 3 for c in ALL_CASES if (c.nx, c.ny) == grid)
        assert any(c.P == 1 for c in ALL_CASES if (c.nx, c.ny) == grid)
        assert all(c.weighted for c in ALL_CASES if (c.nx, c.ny) == grid)
    assert all((c.tilt == wp.TILT) == (c.nz > 1) for c in ALL_CASES) and max(c.nx * c.ny for c in ALL_CASES) <= 256 * 64
    # what the shapes are for: a single partial tile in both kernels; 2.8 step tiles; pairs per row above a tile; the pad pixel
    assert 24 * 20 < wp_tile("ADJ_RES_TILE") and 24 * 10 < wp_tile("ADJ_TILE") and 2 < 45 * 32 / wp_tile("ADJ_TILE") < 3
    assert (1050 + 1) // 2 > wp_tile("ADJ_TILE") and 97 % 2 == 1 and 114 % 2 == 0
    assert wp.GRAD_RESTORE_CASE in wp.GRAD_ODD_CASES


def wp_tile(name):
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "pyslice_amd", "csrc", "adjoint.h")).read()
    per = {"ADJ_RES_TILE": r"ADJ_RES_PER = (\d+), ADJ_RES_TILE = 256 \* ADJ_RES_PER", "ADJ_TILE": r"ADJ_SL = (\d+), ADJ_TILE = 256 \* ADJ_SL"}[name]
    return 256 * int(re.search(per, src).group(1))


def test_step_layout_restates_the_pitch_of_the_library():
    src = open(os.path.join(os.path.dirname(__file__), "..", "pyslice_amd", "csrc", "mslice.hip")).read()
    for line in ("h->pitch = cfg->ny + ((h->Rx || h->Ry) ? pad : 0);",
                 "if (h->pitch == cfg->ny && h->onepass) h->pitch = cfg->ny + 16;",
                 "if (h->onepass && (h->pitch & 1)) ++h->pitch;",
                 "return (h->pitch % 2 == 0) && (((uintptr_t)g & 15) == 0) && (((uintptr_t)h->psi0.p & 15) == 0) && (((uintptr_t)h->adj_stack.p & 15) == 0);"):
        assert line in src, line


def test_layout_accessor_in_the_abi():
    import re
    from pyslice_amd import _native
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "mslice.h")).read()
    assert re.search(r"^int\s+msl_adjoint_layout\(const msl_handle\* h, int32_t\* pitch, int32_t\* vec\);", header, re.M)
    assert "msl_adjoint_layout" in _native.EXPORTS and callable(_native.Engine.adjoint_layout)


@pytest.mark.parametrize("c", ALL_CASES + [wp.GRAD_RESTORE_CASE._replace(tilt=None)], ids=wp.gradient_id)
def test_kappa_cap_and_the_weight(c):
    data = wp.gradient_data(c)
    kap = [float(k) for a in data["adds"] for k in a["kappa"]]
    print(f"{wp.gradient_id(c)}: kappa_loss per probe " + " ".join(f"{k:.2f}" for k in kap))
    assert max(kap) <= wp.KAPPA_CAP and data["kappa"] == max(kap)
    w = data["weight"]
    if c.weighted:
        assert w.dtype == np.float32 and w.min() == 0.0 and 0.9 < w.max() <= 1.0 and 0.2 < (w == 0).mean() < 0.3
        mirrored = w[(-np.arange(c.nx)) % c.nx][:, (-np.arange(c.ny)) % c.ny]
        assert np.abs(w - mirrored).mean() > 0.2 and np.abs(w - w[::-1, ::-1]).mean() > 0.2
    for a in data["adds"]:
        assert a["D"].dtype == np.float32 and a["D"].shape == (a["B"], c.nx, c.ny) and a["probes"].shape == (c.P, c.nx, c.ny)
        assert (np.abs(a["loss"]) > 0).all() and np.abs(a["grad"]).max() > 0


# ---- the loop of msl_adjoint_add, in the precision of the device or in float64, with a fault built in ------------------------------
FAULTS = {
    # name: (case, the ratio to a bound the fault must reach, where: "slices", "probe" or "loss")
    "conj(P) read at -k under tilt":                 (wp.GRAD_ODD_CASES[3], 1e3, "slices"),
    "px / py of the tilt exchanged":                 (wp.GRAD_ODD_CASES[3], 1e3, "slices"),
    "pad pixel as second pixel of an odd row":       (wp.GRAD_ODD_CASES[3], 1e2, "slices"),
    "tail tile not accumulated":                     (wp.GRAD_ODD_CASES[3], 1e2, "slices"),
    "image p with psi of image p + 1":               (wp.GRAD_ODD_CASES[3], 1e3, "slices"),
    "stack slab stride B on the ragged add":         (wp.GRAD_BATCH_CASES[0], 1e3, "slices"),
    "second add overwrites":                         (wp.GRAD_BATCH_CASES[0], 1e3, "slices"),
    "shift off by one along y on odd ny":            (wp.GRAD_ODD_CASES[0], 1e3, "slices"),
    "w read unshifted":                              (wp.GRAD_ODD_CASES[0], 1e3, "slices"),
    "loss of the last residual tile dropped":        (wp.GRAD_ODD_CASES[0], 1e2, "loss"),
    "one accumulator pixel doubled":                 (wp.GRAD_ODD_CASES[3], 10.0, "slices"),
}
# whether the per-slice L1 bound and the loss bound of gradient_cases.py, on the physical inputs, see the fault (measured below and
# asserted, so that the table of DESIGN.md section 4.31 stays true)
OLD_BOUNDS_SEE = {
    "conj(P) read at -k under tilt": False, "px / py of the tilt exchanged": False, "pad pixel as second pixel of an odd row": True,
    "tail tile not accumulated": True, "image p with psi of image p + 1": True, "stack slab stride B on the ragged add": True,
    "second add overwrites": True, "shift off by one along y on odd ny": True, "w read unshifted": True,
    "loss of the last residual tile dropped": True, "one accumulator pixel doubled": False,
}


def loop_model(nx, ny, nz, P, V, weight, eps, loss, adds, tilt, single=True, fault=None, sigma=None, dz=None, dx=None, dy=None):
    """adds: [(probes (P, nx, ny), D (B, nx, ny))] -> (accumulator (nz, nx, ny) float64, [probe gradient per add], [loss per add]).
    single: complex64 waves, float32 transmission, residual factor and per-add sums, float64 loss and accumulator, as the kernels
    of adjoint.h hold them; else float64 throughout"""
    import torch
    from pyslice_amd.tilt import tilted_propagator
    ct, ft = (torch.complex64, torch.float32) if single else (torch.complex128, torch.float64)
    sigma = orc.interaction_sigma(wp.EV) if sigma is None else sigma
    dx, dy, dz = wp.DX if dx is None else dx, wp.DY if dy is None else dy, wp.DZ if dz is None else dz
    tan = tilt
    if fault == "px / py of the tilt exchanged" and tilt is not None:
        tan = (tilt[1], tilt[0])
    fwd = torch.from_numpy(tilted_propagator(nx, ny, dx, dy, orc.wavelength(wp.EV), dz, wp.tilt_object(tilt))).to(ct)
    back = torch.conj(torch.from_numpy(tilted_propagator(nx, ny, dx, dy, orc.wavelength(wp.EV), dz, wp.tilt_object(tan))).to(ct))
    if fault == "conj(P) read at -k under tilt":
        back = torch.roll(torch.flip(back, (0, 1)), (1, 1), (0, 1))
    ph = torch.from_numpy(np.array(V)).to(ft) * torch.tensor(sigma, dtype=ft)
    t = torch.complex(torch.cos(ph), torch.sin(ph))
    wu = None if weight is None else torch.from_numpy(np.array(weight if fault == "w read unshifted" else np.fft.ifftshift(weight))).to(ft)
    off_y = fault == "shift off by one along y on odd ny" and ny % 2 == 1
    if off_y and wu is not None:
        wu = torch.roll(wu, 1, 1)
    ppr = (ny + 1) // 2
    pair_q = torch.arange(nx)[:, None] * ppr + torch.arange(ny)[None, :] // 2
    tail = pair_q >= (((nx * ppr + 511) // 512) - 1) * 512
    pix_q = torch.arange(nx)[:, None] * ny + torch.arange(ny)[None, :]
    res_tail = pix_q >= (((nx * ny + 1023) // 1024) - 1) * 1024
    acc = torch.zeros((nz, nx, ny), dtype=torch.float64)
    pgs, losses = [], []
    for n_add, (probes, D) in enumerate(adds):
        B = len(D)
        psi = torch.from_numpy(np.array(probes)).to(ct)
        stack = []
        for s in range(nz):
            if s > 0:
                stack.append(psi)
            phi = t[s] * psi
            if s < nz - 1:
                psi = torch.fft.ifft2(fwd * torch.fft.fft2(phi))
        stack = torch.stack(stack) if stack else None                   # (nz - 1, P, nx, ny)
        Psi = torch.fft.fft2(phi)[:B]
        Du = torch.from_numpy(np.fft.ifftshift(np.asarray(D), axes=AX)).to(ft)
        if off_y:
            Du = torch.roll(Du, 1, 2)
        I = Psi.real ** 2 + Psi.imag ** 2
        w1 = 1.0 if wu is None else wu
        I64, D64 = I.double(), Du.double()
        w64 = 1.0 if wu is None else wu.double()
        if loss == "amplitude":
            a, sd = torch.sqrt(I), torch.sqrt(Du)
            f = w1 * (1.0 - sd / torch.clamp(a, min=float(np.sqrt(eps))))
            terms = w64 * (a.double() - sd.double()) ** 2
        elif loss == "intensity":
            f = w1 * (I - Du)
            terms = 0.5 * w64 * (I64 - D64) ** 2
        else:
            f = w1 * (1.0 - Du / (I + eps))
            terms = w64 * (I64 - D64 * torch.log(I64 + eps))
        if fault == "loss of the last residual tile dropped":
            terms = terms * (~res_tail)
        losses.append(terms.sum(dim=AX).numpy())
        g = torch.fft.ifft2((f * Psi).to(ct), norm="forward")
        share = torch.zeros((nz, nx, ny), dtype=torch.float64)
        for s in range(nz - 1, -1, -1):
            if s == 0:
                ps = torch.from_numpy(np.array(probes)).to(ct)
            elif fault == "stack slab stride B on the ragged add":
                flat = stack.reshape(-1, nx, ny)
                ps = torch.cat([flat[(s - 1) * B:(s - 1) * B + B], flat[:max(0, len(probes) - B)]])
            else:
                ps = stack[s - 1]
            if fault == "image p with psi of image p + 1":
                ps = torch.roll(ps, -1, 0)
            phi = t[s] * ps[:B]
            sums = torch.zeros((nx, ny), dtype=ft)
            for p in range(B):
                sums = sums + (g[p].imag * phi[p].real - g[p].real * phi[p].imag)
            if fault == "tail tile not accumulated":
                sums = sums * (~tail)
            if fault == "pad pixel as second pixel of an odd row" and ny % 2 == 1:
                # the pad behind row x taken to hold the row's last pixel; its product lands on grad[pix + 1], pixel (x + 1, 0)
                pad = (g[:, :-1, -1] * torch.conj(t[s][1:, 0] * ps[:B, :-1, -1])).imag.sum(dim=0)
                sums[1:, 0] = sums[1:, 0] + pad
            share[s] = 2.0 * sigma * sums.double()
            g = torch.conj(t[s]) * g
            if s > 0:
                g = torch.fft.ifft2(back * torch.fft.fft2(g))
        acc = share if (fault == "second add overwrites" and n_add > 0) else acc + share
        pgs.append(g.numpy())
    acc = acc.numpy()
    if fault == "one accumulator pixel doubled":
        s0 = nz - 1
        i = np.unravel_index(np.argsort(np.abs(acc[s0]).ravel())[acc[s0].size // 2], acc[s0].shape)     # a pixel of median modulus
        acc[(s0,) + i] *= 2.0
    return acc, pgs, losses


def run_model(c, fault=None, single=True):
    data = wp.gradient_data(c)
    got = loop_model(c.nx, c.ny, c.nz, c.P, data["V"], data["weight"], data["epsilon"], c.loss, [(a["probes"], a["D"]) for a in data["adds"]],
                     c.tilt, single=single, fault=fault)
    return data, got


def test_the_float64_model_is_the_definition():
    for c in (wp.GRAD_ODD_CASES[2], wp.GRAD_BATCH_CASES[1], wp.GRAD_SINGLE_TILE_CASES[0]):
        data, got = run_model(c, single=False)
        res = wp.gradient_compare(c, data, *got)
        print(f"{wp.gradient_id(c)} float64 model: worst figure / bound {res['worst']:.2e}")
        assert res["worst"] < 1e-6


@pytest.mark.parametrize("c", ALL_CASES + [wp.GRAD_RESTORE_CASE._replace(tilt=None)], ids=wp.gradient_id)
def test_complex64_model_is_inside_a_third_of_every_bound(c):
    data, got = run_model(c)
    res = wp.gradient_compare(c, data, *got)
    so, po = np.max(res["slices_of"], axis=0), np.max(res["probe_of"], axis=0)
    print(f"{wp.gradient_id(c)}: accumulator of bound " + " ".join(f"{v:.3f}" for v in so) + " | probe gradient " + " ".join(f"{v:.3f}" for v in po) +
          f" | loss {max(v.max() for v in res['loss_of']):.3f} | figures " + " ".join(f"{v:.2e}" for v in np.max(res["slices"], axis=0)))
    assert res["worst"] <= 1.0 / 3.0
    if c.tilt is not None:
        moved = wp.gradient_moved(c, data, got[0], got[1][0])
        print(f"{wp.gradient_id(c)}: moved {moved[0]:.2f} {moved[1]:.2f}")
        assert min(moved) > 0.5


def old_l1_of_bound(data, acc):
    """the per-slice bound of gradient_cases.gradient_bound, on a white case: ||got_s - want_s||_1 over 3 EPS 2 sigma sum_p ||g||_2 ||phi||_2"""
    out = []
    for s in range(len(acc)):
        b = 3.0 * gc.EPS * 2.0 * data["sigma"] * sum(np.linalg.norm(g[p]) * np.linalg.norm(phi[p]) for a in data["adds"] for g, phi in [a["pairs"][s]] for p in range(len(g)))
        out.append(np.abs(acc[s] - data["grad"][s]).sum() / b)
    return max(out)


@pytest.mark.parametrize("fault", list(FAULTS), ids=[f.replace(" ", "_") for f in FAULTS])
def test_each_fault_exceeds_a_bound_by_its_factor(fault):
    c, factor, where = FAULTS[fault]
    data, got = run_model(c, fault=fault)
    res = wp.gradient_compare(c, data, *got)
    ratios = dict(slices=float(np.max(res["slices_of"])), probe=float(np.max(res["probe_of"])), loss=float(max(v.max() for v in res["loss_of"])))
    old = old_l1_of_bound(data, got[0])
    print(f"{fault} ({wp.gradient_id(c)}): accumulator {ratios['slices']:.3g} x, probe gradient {ratios['probe']:.3g} x, loss {ratios['loss']:.3g} x its bound; "
          f"pixel {np.max(res['slices_of'], axis=0)[2]:.3g} x; the L1 bound of gradient_cases on this input {old:.3g} x")
    assert ratios[where] >= factor
    if fault == "one accumulator pixel doubled":
        assert np.max(res["slices_of"], axis=0)[2] >= 10.0 and old <= 1.0


@pytest.fixture(scope="module")
def physical():
    """the inputs of test_gpu_gradient.py at 101 x 97 x 4 as the calculator feeds them at probe_batch=2: adds of (2, 1), the ragged
    batch padded with its last probe"""
    grid = (101, 97, 4)
    c = gc.case(*grid)
    pr = c["probes"]
    adds = [(pr[0:2], c["D"][0:2]), (np.stack([pr[2], pr[2]]), c["D"][2:3])]
    return grid, c, adds


@pytest.mark.parametrize("fault", list(FAULTS), ids=[f.replace(" ", "_") for f in FAULTS])
def test_what_the_aggregate_bounds_on_the_physical_inputs_see(physical, fault):
    """the fault in the float64 model on the inputs of test_gpu_gradient.py, against its per-slice L1 bound and its loss bound (the
    weighted run for the faults of the weight and the shift): a ratio above 1 is seen"""
    grid, c, adds = physical
    weighted = fault in ("w read unshifted", "shift off by one along y on odd ny")
    ref = gc.reference(*grid, weighted=weighted)
    w = gc.disc_weight(grid[0], grid[1]) if weighted else None
    geo = dict(sigma=c["sigma"], dz=float(c["zs"][1] - c["zs"][0]), dx=float(c["xs"][1] - c["xs"][0]), dy=float(c["ys"][1] - c["ys"][0]))
    acc, _, losses = loop_model(*grid, 2, c["V"], w, 1e-20, "amplitude", adds, None, single=False, fault=fault, **geo)
    clean = loop_model(*grid, 2, c["V"], w, 1e-20, "amplitude", adds, None, single=False, **geo)
    assert (np.abs(clean[0] - ref["grad"]).sum(axis=AX) <= 1e-6 * gc.gradient_bound(c, ref)).all()
    g_ratio = float((np.abs(acc - ref["grad"]).sum(axis=AX) / gc.gradient_bound(c, ref)).max())
    l_ratio = float((np.abs(np.concatenate(losses) - ref["loss"]) / gc.loss_bound(c, ref, "amplitude")).max())
    seen = max(g_ratio, l_ratio) > 1.0
    print(f"{fault}: physical inputs {grid}: gradient L1 / bound {g_ratio:.3g}, loss / bound {l_ratio:.3g}: {'seen' if seen else 'NOT seen'}")
    assert seen == OLD_BOUNDS_SEE[fault]


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
class Float64AdjointEngine:
    """the calls of gradient_case() on pyslice_amd/adjoint.py; ignore_tilt: set_tilt does nothing"""

    def __init__(self, nx, ny, nz, P, ignore_tilt=False, **kw):
        self.shape, self.P, self.kw, self.ignore_tilt = (nx, ny, nz), P, kw, ignore_tilt
        self.calls, self.tilt = [], None

    def upload_probes(self, arr):
        assert arr.shape == (self.P,) + self.shape[:2]
        self.calls.append("upload_probes")
        self.probes = arr

    def upload_potential(self, V):
        self.calls.append("upload_potential")
        self.V = V.astype(np.float64)

    def set_tilt(self, tx, ty):
        self.calls.append(f"set_tilt {tx:g} {ty:g}")
        if not self.ignore_tilt:
            self.tilt = (tx, ty)

    def set_adjoint(self, kind, eps, weight):
        from pyslice_amd.adjoint import LOSSES
        self.calls.append("set_adjoint")
        self.loss = {v: k for k, v in LOSSES.items()}[kind]
        self.eps, self.w = eps, weight
        self.acc = np.zeros((self.shape[2],) + self.shape[:2])

    def adjoint_layout(self):
        return wp.step_layout(self.shape[0], self.shape[1], self.kw.get("fft_path", 0))

    def adjoint_reset(self):
        self.calls.append("adjoint_reset")
        self.acc[:] = 0.0

    def adjoint_add(self, data, B=None, probe=False):
        from pyslice_amd.adjoint import potential_gradient
        from pyslice_amd.tilt import tilted_propagator
        self.calls.append(f"adjoint_add {B}")
        nx, ny, _ = self.shape
        prop = tilted_propagator(nx, ny, wp.DX, wp.DY, orc.wavelength(wp.EV), wp.DZ, wp.tilt_object(self.tilt))
        grad, L, pg = potential_gradient(self.probes[:B], self.V, data, orc.interaction_sigma(wp.EV), prop, self.loss, self.w, self.eps)
        self.acc += grad
        return L, pg.astype(np.complex64)

    def adjoint_download(self):
        self.calls.append("adjoint_download")
        return self.acc.copy()

    def close(self):
        self.calls.append("close")


def test_gradient_case_plumbing_on_a_float64_engine(monkeypatch):
    made = []

    def fake(**extra):
        def make(nx, ny, nz, P, **kw):
            made.append(Float64AdjointEngine(nx, ny, nz, P, **extra, **kw))
            return made[-1]
        return make
    monkeypatch.setattr(wp, "engine", fake())
    c = wp.GRAD_BATCH_CASES[0]
    res = wp.gradient_case(c)
    assert made[-1].calls == ["upload_probes", "upload_potential", "set_tilt 0.17 -0.11", "set_adjoint", "upload_probes", "adjoint_add 3",
                              "upload_probes", "adjoint_add 2", "adjoint_download", "close"]
    assert res["worst"] < 1e-2 and (res["pitch"], res["vec"]) == (63, False) and min(res["moved"]) > 0.5 and made[-1].kw["fft_path"] == 1
    assert len(res["probe"]) == 2 and len(res["slices"]) == 3 and [len(v) for v in res["loss_of"]] == [3, 2]
    res = wp.gradient_case(wp.GRAD_RESTORE_CASE, restore=True)
    assert made[-1].calls[-6:] == ["set_tilt 0 0", "adjoint_reset", "upload_probes", "adjoint_add 2", "adjoint_download", "close"]
    assert res["worst"] < 1e-2 and res["restored"]["worst"] < 1e-2 and res["vec"] is True
    # a tilt that never reaches the handle: far above every bound, and not moved
    monkeypatch.setattr(wp, "engine", fake(ignore_tilt=True))
    res = wp.gradient_case(wp.GRAD_RESTORE_CASE)
    assert res["worst"] > 1e3 and max(res["moved"]) < 1e-2

"""The host side of MultisliceCalculator on an engine that only records its calls: every run mode issues the sequence of engine
calls written out below, and the engine is sized by the memory rules as written out below.  Both sets of literals were taken from
the calculator as it was before its set-up and loops were folded into shared helpers; they are compared for equality."""
import pytest

from recording_engine import RecordingEngine, format_calls

PP = [(0.3 * i, 0.2 * i) for i in range(7)]
GRID = "32, 32, 3, 0.0984375, 0.0984375, 0.416666666667, 0.0370143628314, 0.000924395920681"      # nx, ny, nz, dx, dy, dz, wavelength, sigma


def _trajectory(n_frames):
    from pyslice_amd.synthetic import synthetic_trajectory
    return synthetic_trajectory(32, 3, n_frames, density=0.05, seed=4)


def _modes():
    from pyslice_amd import Aberrations, Detector, Diffraction
    dets = [Detector("bf", outer=20.0), Detector("adf", inner=40.0)]
    dif = Diffraction(bin=(4, 8))
    split = Diffraction(bin=(4, 8), split=True)
    # name: (constructor arguments, frames, run method)
    cases = {"run_fb1": (dict(frame_batch=1), 5, "run"),
             "run_fb2": (dict(frame_batch=2), 5, "run"),
             "run_refused_with_stream_tile": (dict(stream_tile=2, frame_batch=2), 5, "run"),
             "stream_fb1": (dict(stream_tile=2, frame_batch=1), 5, "run_streaming_tacaw"),
             "stream_fb2": (dict(stream_tile=2, frame_batch=2), 5, "run_streaming_tacaw"),
             "aberrations": (dict(frame_batch=2, aberrations=Aberrations(defocus=100.0)), 5, "run"),
             "k_window": (dict(frame_batch=2, k_window=(16, 8)), 5, "run")}
    for fb in (1, 2):
        cases[f"detectors_fb{fb}"] = (dict(detectors=dets, probe_batch=3, frame_batch=fb), 3, "run_detectors")
        cases[f"diffraction_fb{fb}"] = (dict(diffraction=dif, probe_batch=3, frame_batch=fb), 3, "run_diffraction")
        cases[f"diffraction_detectors_fb{fb}"] = (dict(diffraction=dif, detectors=dets, probe_batch=3, frame_batch=fb), 3, "run_diffraction")
    for T, fb in ((5, 2), (2, 2), (3, 1)):
        cases[f"split_{T}_fb{fb}"] = (dict(diffraction=split, probe_batch=3, frame_batch=fb), T, "run_diffraction")
    return cases


CASES = ["run_fb1", "run_fb2", "run_refused_with_stream_tile", "stream_fb1", "stream_fb2", "detectors_fb1", "detectors_fb2",
         "diffraction_fb1", "diffraction_fb2", "diffraction_detectors_fb1", "diffraction_detectors_fb2", "split_5_fb2", "split_2_fb2",
         "split_3_fb1", "aberrations", "k_window"]


def trace(name):
    """the engine calls of one case as lines of text (with _native.Engine already replaced by the recorder)"""
    from pyslice_amd.calculators import MultisliceCalculator
    kw, n_frames, method = _modes()[name]
    calc = MultisliceCalculator(progress=False, **kw)
    calc.setup(_trajectory(n_frames), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
    try:
        getattr(calc, method)()
        end = []
    except RuntimeError as e:
        end = [f"RuntimeError: {e}"]
    eng = calc._engine
    lines = format_calls([eng.created] + eng.calls, PP) + end
    return [lines[0].replace(GRID, "GRID")] + lines[1:]


class CountingEngine(RecordingEngine):
    """records the (n_probes, n_frames, frame_batch) of every construction and fails the first `failures` of them"""
    attempts, failures = [], 0

    def __init__(self, *a, **k):
        CountingEngine.attempts.append((k["n_probes"], k["n_frames"], k["frame_batch"]))
        if len(CountingEngine.attempts) <= CountingEngine.failures:
            raise MemoryError("no room")
        super().__init__(*a, **k)


SIZING = {"resident": dict(), "stream_tile": dict(stream_tile=4), "probe_batches": "plain", "probe_batches_split": "split"}


def sizing(kind, failures=0, **explicit):
    """the engine constructions setup() attempts for 7 probes x 8 frames in one of the SIZING modes (with _native.Engine already
    replaced by CountingEngine), and whether it gave up"""
    from pyslice_amd import Diffraction
    from pyslice_amd.calculators import MultisliceCalculator
    kw = SIZING[kind]
    if isinstance(kw, str):
        kw = dict(diffraction=Diffraction(bin=(4, 8), split=kw == "split"))
    CountingEngine.attempts, CountingEngine.failures = [], failures
    calc = MultisliceCalculator(progress=False, **kw, **explicit)
    try:
        calc.setup(_trajectory(8), aperture=30.0, voltage_eV=100e3, probe_positions=PP)
        return CountingEngine.attempts, "ok"
    except MemoryError:
        return CountingEngine.attempts, "MemoryError"


# ------------------------------------------------------------------ 1. the engine sees the same calls
EXPECTED = {
    "run_fb1": [
        "Engine(GRID, n_probes=7, n_frames=5, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(0)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(1)", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(2)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(3)", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(4)", "synchronize()", "wavefunction_c128(5)"],
    "run_fb2": [
        "Engine(GRID, n_probes=7, n_frames=5, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])", "build_potentials(f8(2,2,3), i4(2,), 2)",
        "propagate_frames(0, 2)", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(2, 2)", "build_potentials(f8(1,2,3), i4(2,), 2)",
        "propagate_frames(4, 1)", "synchronize()", "wavefunction_c128(5)"],
    "run_refused_with_stream_tile": [
        "Engine(GRID, n_probes=7, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])",
        "RuntimeError: stream_tile is set: the device holds a ring of frames only -- call run_streaming_tacaw()"],
    "stream_fb1": [
        "Engine(GRID, n_probes=7, n_frames=2, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])", "tacaw_stream_begin(5, i8(5,))",
        "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(1)",
        "tacaw_stream_set_reference(slot=0)", "tacaw_stream_push(0, 2, 0)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)",
        "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(1)", "tacaw_stream_push(0, 2, 2)", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(0)", "tacaw_stream_push(0, 1, 4)", "tacaw_stream_finish(True)", "intensity()"],
    "stream_fb2": [
        "Engine(GRID, n_probes=7, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])", "tacaw_stream_begin(5, i8(5,))",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "tacaw_stream_set_reference(slot=0)", "tacaw_stream_push(0, 2, 0)",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "tacaw_stream_push(0, 2, 2)", "build_potentials(f8(1,2,3), i4(2,), 2)",
        "propagate_frames(0, 1)", "tacaw_stream_push(0, 1, 4)", "tacaw_stream_finish(True)", "intensity()"],
    "detectors_fb1": [
        "Engine(GRID, n_probes=3, n_frames=1, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_detectors(u2(1024,), (intensity,intensity), f4(32,), f4(32,))",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])",
        "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "detect(0, 1, B=1)",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])",
        "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "detect(0, 1, B=1)",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])",
        "propagate_frame(0)", "detect(0, 1, B=3)", "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "detect(0, 1, B=1)"],
    "detectors_fb2": [
        "Engine(GRID, n_probes=3, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_detectors(u2(1024,), (intensity,intensity), f4(32,), f4(32,))",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frames(0, 2)", "detect(0, 2, B=3)",
        "set_probes(30, xy[3,4,5])", "propagate_frames(0, 2)", "detect(0, 2, B=3)", "set_probes(30, xy[6,6,6])", "propagate_frames(0, 2)",
        "detect(0, 2, B=1)", "build_potentials(f8(1,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frames(0, 1)", "detect(0, 1, B=3)",
        "set_probes(30, xy[3,4,5])", "propagate_frames(0, 1)", "detect(0, 1, B=3)", "set_probes(30, xy[6,6,6])", "propagate_frames(0, 1)",
        "detect(0, 1, B=1)"],
    "diffraction_fb1": [
        "Engine(GRID, n_probes=3, n_frames=1, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])",
        "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))",
        "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "diffract(0, 1, B=1, bin=(4,8))", "build_potential(f8(2,3), i4(2,), 2)",
        "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "propagate_frame(0)",
        "diffract(0, 1, B=3, bin=(4,8))", "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "diffract(0, 1, B=1, bin=(4,8))",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))",
        "set_probes(30, xy[3,4,5])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "set_probes(30, xy[6,6,6])", "propagate_frame(0)",
        "diffract(0, 1, B=1, bin=(4,8))"],
    "diffraction_fb2": [
        "Engine(GRID, n_probes=3, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "build_potentials(f8(2,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])",
        "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "propagate_frames(0, 2)",
        "diffract(0, 2, B=3, bin=(4,8))", "set_probes(30, xy[6,6,6])", "propagate_frames(0, 2)", "diffract(0, 2, B=1, bin=(4,8))",
        "build_potentials(f8(1,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))",
        "set_probes(30, xy[3,4,5])", "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))", "set_probes(30, xy[6,6,6])",
        "propagate_frames(0, 1)", "diffract(0, 1, B=1, bin=(4,8))"],
    "diffraction_detectors_fb1": [
        "Engine(GRID, n_probes=3, n_frames=1, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_detectors(u2(1024,), (intensity,intensity), f4(32,), f4(32,))",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))",
        "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "detect(0, 1, B=3)",
        "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "diffract(0, 1, B=1, bin=(4,8))", "detect(0, 1, B=1)",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))",
        "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "detect(0, 1, B=3)",
        "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "diffract(0, 1, B=1, bin=(4,8))", "detect(0, 1, B=1)",
        "build_potential(f8(2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))",
        "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "detect(0, 1, B=3)",
        "set_probes(30, xy[6,6,6])", "propagate_frame(0)", "diffract(0, 1, B=1, bin=(4,8))", "detect(0, 1, B=1)"],
    "diffraction_detectors_fb2": [
        "Engine(GRID, n_probes=3, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_detectors(u2(1024,), (intensity,intensity), f4(32,), f4(32,))",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))",
        "detect(0, 2, B=3)", "set_probes(30, xy[3,4,5])", "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "detect(0, 2, B=3)",
        "set_probes(30, xy[6,6,6])", "propagate_frames(0, 2)", "diffract(0, 2, B=1, bin=(4,8))", "detect(0, 2, B=1)",
        "build_potentials(f8(1,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])", "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))",
        "detect(0, 1, B=3)", "set_probes(30, xy[3,4,5])", "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))", "detect(0, 1, B=3)",
        "set_probes(30, xy[6,6,6])", "propagate_frames(0, 1)", "diffract(0, 1, B=1, bin=(4,8))", "detect(0, 1, B=1)"],
    "split_5_fb2": [
        "Engine(GRID, n_probes=3, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2])", "coherent_reset()",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)",
        "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)",
        "build_potentials(f8(1,2,3), i4(2,), 2)", "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)",
        "coherent_finish(5, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "coherent_reset()", "build_potentials(f8(2,2,3), i4(2,), 2)",
        "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)", "build_potentials(f8(2,2,3), i4(2,), 2)",
        "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)", "build_potentials(f8(1,2,3), i4(2,), 2)",
        "propagate_frames(0, 1)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)", "coherent_finish(5, B=3, bin=(4,8))",
        "set_probes(30, xy[6,6,6])", "coherent_reset()", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)",
        "diffract(0, 2, B=1, bin=(4,8))", "coherent_add(0, 2, B=1)", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(0, 2)",
        "diffract(0, 2, B=1, bin=(4,8))", "coherent_add(0, 2, B=1)", "build_potentials(f8(1,2,3), i4(2,), 2)", "propagate_frames(0, 1)",
        "diffract(0, 1, B=1, bin=(4,8))", "coherent_add(0, 1, B=1)", "coherent_finish(5, B=1, bin=(4,8))"],
    "split_2_fb2": [
        "Engine(GRID, n_probes=3, n_frames=2, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "build_potentials(f8(2,2,3), i4(2,), 2)", "set_probes(30, xy[0,1,2])",
        "coherent_reset()", "propagate_frames(0, 2)", "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)",
        "coherent_finish(2, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "coherent_reset()", "propagate_frames(0, 2)",
        "diffract(0, 2, B=3, bin=(4,8))", "coherent_add(0, 2, B=3)", "coherent_finish(2, B=3, bin=(4,8))", "set_probes(30, xy[6,6,6])",
        "coherent_reset()", "propagate_frames(0, 2)", "diffract(0, 2, B=1, bin=(4,8))", "coherent_add(0, 2, B=1)",
        "coherent_finish(2, B=1, bin=(4,8))"],
    "split_3_fb1": [
        "Engine(GRID, n_probes=3, n_frames=1, frame_batch=1, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2])", "coherent_reset()",
        "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)",
        "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)",
        "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)",
        "coherent_finish(3, B=3, bin=(4,8))", "set_probes(30, xy[3,4,5])", "coherent_reset()", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)", "build_potential(f8(2,3), i4(2,), 2)",
        "propagate_frame(0)", "diffract(0, 1, B=3, bin=(4,8))", "coherent_add(0, 1, B=3)", "coherent_finish(3, B=3, bin=(4,8))",
        "set_probes(30, xy[6,6,6])", "coherent_reset()", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)",
        "diffract(0, 1, B=1, bin=(4,8))", "coherent_add(0, 1, B=1)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)",
        "diffract(0, 1, B=1, bin=(4,8))", "coherent_add(0, 1, B=1)", "build_potential(f8(2,3), i4(2,), 2)", "propagate_frame(0)",
        "diffract(0, 1, B=1, bin=(4,8))", "coherent_add(0, 1, B=1)", "coherent_finish(3, B=1, bin=(4,8))"],
    "aberrations": [
        "Engine(GRID, n_probes=7, n_frames=5, frame_batch=2, window=None, k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(Aberrations)", "set_probes(30, xy[0,1,2,3,4,5,6])", "build_potentials(f8(2,2,3), i4(2,), 2)",
        "propagate_frames(0, 2)", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(2, 2)", "build_potentials(f8(1,2,3), i4(2,), 2)",
        "propagate_frames(4, 1)", "synchronize()", "wavefunction_c128(5)"],
    "k_window": [
        "Engine(GRID, n_probes=7, n_frames=5, frame_batch=2, window=(16,8), k_bin=None, device=0)", "set_kirkland(f8(103,3,4))",
        "set_slices(f8(3,), f8(3,))", "set_aberrations(None)", "set_probes(30, xy[0,1,2,3,4,5,6])", "build_potentials(f8(2,2,3), i4(2,), 2)",
        "propagate_frames(0, 2)", "build_potentials(f8(2,2,3), i4(2,), 2)", "propagate_frames(2, 2)", "build_potentials(f8(1,2,3), i4(2,), 2)",
        "propagate_frames(4, 1)", "synchronize()", "wavefunction_c128(5)"],
}


@pytest.mark.parametrize("name", CASES)
def test_engine_calls(monkeypatch, name):
    """method names, order, counts, B=, slot and count arguments, the shapes of the arrays, the probes of every set_probes by
    their index (the last batch padded with its last position)"""
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", RecordingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    assert trace(name) == EXPECTED[name]


# ------------------------------------------------------------------ 2. the sizing policy
_ROOM = dict(unlimited=300e9, one_halving=2.1074e9, down_to_one=2.0e9, unknown=None)
_ROOM_PB = dict(unlimited=300e9, room_without_split_only=1.11416e9, one_halving=1.1135e9, down_to_one=1.0e9, unknown=None)
FREE = {"resident": _ROOM, "stream_tile": dict(_ROOM, one_halving=2.1065e9), "probe_batches": _ROOM_PB, "probe_batches_split": _ROOM_PB}
SIZED = {"resident": dict(unlimited=(7, 8, 8), one_halving=(7, 8, 4), down_to_one=(7, 8, 1), unknown=(7, 8, 8)),
         "stream_tile": dict(unlimited=(7, 4, 4), one_halving=(7, 4, 2), down_to_one=(7, 4, 1), unknown=(7, 4, 4)),
         "probe_batches": dict(unlimited=(7, 8, 8), room_without_split_only=(7, 8, 8), one_halving=(3, 8, 8), down_to_one=(1, 8, 8),
                               unknown=(7, 8, 8)),
         "probe_batches_split": dict(unlimited=(7, 8, 8), room_without_split_only=(3, 8, 8), one_halving=(3, 8, 8), down_to_one=(1, 8, 8),
                                     unknown=(7, 8, 8))}


@pytest.mark.parametrize("kind", list(SIZING))
def test_preflight_sizing(monkeypatch, kind):
    """free device memory -> the (n_probes, n_frames, frame_batch) the engine is created with"""
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", CountingEngine)
    for label, free_b in FREE[kind].items():
        monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: free_b)
        assert sizing(kind) == ([SIZED[kind][label]], "ok"), label


_PB_RETRIES = {1: ([(7, 8, 8), (3, 8, 8)], "ok"), 2: ([(7, 8, 8), (3, 8, 8), (1, 8, 8)], "ok"),
               3: ([(7, 8, 8), (3, 8, 8), (1, 8, 8), (1, 4, 4)], "ok")}              # the probe batch first, then the frame batch
RETRIES = {"resident": {1: ([(7, 8, 8), (7, 8, 4)], "ok"), 2: ([(7, 8, 8), (7, 8, 4), (7, 8, 2)], "ok"),
                        3: ([(7, 8, 8), (7, 8, 4), (7, 8, 2), (7, 8, 1)], "ok")},
           "stream_tile": {1: ([(7, 4, 4), (7, 4, 2)], "ok"), 2: ([(7, 4, 4), (7, 4, 2), (7, 4, 1)], "ok"),
                           3: ([(7, 4, 4), (7, 4, 2), (7, 4, 1)], "MemoryError")},
           "probe_batches": _PB_RETRIES, "probe_batches_split": _PB_RETRIES}


@pytest.mark.parametrize("kind", list(SIZING))
def test_memory_error_retries(monkeypatch, kind):
    """an engine that does not fit is tried again smaller: the sequence of attempts after one, two and three failures"""
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", CountingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: None)
    for failures in (1, 2, 3):
        got = sizing(kind, failures)
        assert got == RETRIES[kind][failures], failures


@pytest.mark.parametrize("kind,explicit,first", [("resident", dict(frame_batch=4), (7, 8, 4)), ("stream_tile", dict(frame_batch=4), (7, 4, 4)),
                                                 ("probe_batches", dict(probe_batch=4), (4, 8, 8)),
                                                 ("probe_batches_split", dict(probe_batch=4), (4, 8, 8))])
def test_explicit_sizes_are_not_shrunk(monkeypatch, kind, explicit, first):
    from pyslice_amd import _native, calculators
    monkeypatch.setattr(_native, "Engine", CountingEngine)
    monkeypatch.setattr(calculators, "_free_device_bytes", lambda dev: 1.0)          # (no pre-flight halving either)
    assert sizing(kind, 1, **explicit) == ([first], "MemoryError")

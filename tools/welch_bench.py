"""Time msl_tacaw_welch alone: (P, T, npix) complex64 random spectra resident on the device -> (P, L, npix) float32 Welch intensity,
next to msl_tacaw on the same array.

    python tools/welch_bench.py --frames 256 --welch 128,64 [--welch 128,128 --welch 64,32] [--probes 16] [--pixels 1048576] [--reps 5]

Prints ms per call and the rate on the byte model 8 S L npix read + 4 L npix written per image (S = 1 + (T - L) // hop; overlapping
segments count every read).  Used under rocprofv3 for the kernel trace and, in a run of its own, FETCH_SIZE of time_welch_kernel:
FETCH_SIZE below the model's read bytes at hop = L / 2 means the re-read half comes from L2 / MALL."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--pixels", type=int, default=1024 * 1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--welch", action="append", default=None, metavar="L,HOP", help="segment length and hop (repeatable)")
    ap.add_argument("--window", default="hann")
    ap.add_argument("--no-tacaw", action="store_true", help="skip the msl_tacaw comparison run")
    a = ap.parse_args()
    import torch
    from pyslice_amd import _native, welch
    P, T, K = a.probes, a.frames, a.pixels
    cases = [tuple(int(v) for v in c.split(",")) for c in (a.welch or ["128,64"])]
    dev = torch.device("cuda", 0)
    src = torch.view_as_complex(torch.randn((P, T, K, 2), dtype=torch.float32, device=dev))
    dst = torch.empty((P, T, K), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng = _native.Engine(2, 2, 1, 1.0, 1.0, 1.0, 1.0, 0.0, n_probes=1, n_frames=0, device=0)

    def timed(call):
        call()                                                  # tables, warm-up
        ms = []
        for _ in range(a.reps):
            before = eng.counters()["ms_tacaw"]
            call()
            ms.append(eng.counters()["ms_tacaw"] - before)
        return min(ms), ms
    if not a.no_tacaw:
        best, ms = timed(lambda: eng.tacaw(src.data_ptr(), dst.data_ptr(), P, T, K))
        print(f"msl_tacaw T={T} P={P} npix={K}: {best:.3f} ms (min of {a.reps}; all: {' '.join('%.2f' % m for m in ms)}) = "
              f"{12.0 * P * T * K / best / 1e6:.0f} GB/s = {12.0 * P * T * K / best / 1e6 / HBM_PEAK_GBS:.3f} of the HBM peak", flush=True)
    for L, hop in cases:
        S = welch.segments(T, L, hop)
        w = welch.window(a.window, L)
        nbytes = float(P) * K * (8.0 * S * L + 4.0 * L)
        best, ms = timed(lambda: eng.tacaw_welch(L, hop, w, src.data_ptr(), dst.data_ptr(), P, T, K))
        print(f"msl_tacaw_welch T={T} L={L} hop={hop} S={S} {a.window} P={P} npix={K}: {best:.3f} ms (min of {a.reps}; all: "
              f"{' '.join('%.2f' % m for m in ms)}) = {nbytes / best / 1e6:.0f} GB/s = {nbytes / best / 1e6 / HBM_PEAK_GBS:.3f} of the HBM peak "
              f"on {nbytes / 1e9:.2f} GB (read {8.0 * S * L * P * K / 1e9:.2f}, written {4.0 * L * P * K / 1e9:.2f})", flush=True)
    eng.close()


if __name__ == "__main__":
    main()

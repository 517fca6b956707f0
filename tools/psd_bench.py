"""Rates of sgx_psd_batch / sgx_csd_batch (PCM to Welch-averaged spectra per bin over groups of frames) against what the same result
costs with the entry points the library had before: sgx_stft_batch (or sgx_stft_batch_complex) in 2 GiB chunks of stored rows and a
torch square / mean (or products / mean) over the group on them -- and against the bare row store as that leg's lower bound.  The legs
are timed interleaved on one device, every iteration kept.  One JSON line per workload and leg: the median rate, the spread of the
iterations (p10 .. p90 and min .. max, as rates).  The first `--settle` seconds of iterations load the device and are not counted.
Where sgx_psd_fused / sgx_csd_fused answer 1 a leg with SGX_FLAG_NO_FUSED_RENDER (the workspace route) runs beside the fused one; where
they answer 0 the call is the workspace route and there is one leg.

    python tools/psd_bench.py [--iters 40] [--settle 3] [--group 256] [--frames 1000000] [--case psd_mono ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {   # name: (W, H, channels, cross)
    "psd_mono": (2048, 256, 1, False),
    "psd_lr": (2048, 256, 2, False),
    "csd_lr": (2048, 256, 2, True),
}
CHUNK_BYTES = 2 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--settle", type=float, default=3.0, help="seconds of interleaved iterations before the counted ones")
    ap.add_argument("--group", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch, cross = CASES[name]
        frames, group = a.frames, a.group
        kw = dict(window_samples=W, hop_samples=H, channels=ch, device=0)
        eng, split = SpectrogramEngine(48000.0, **kw), SpectrogramEngine(48000.0, fused_render=False, **kw)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        comps = 4 if cross else 2
        cols = -(-frames // group)
        out = torch.empty((cols, eng.pairs, eng.M, comps), dtype=torch.float32, device=eng.device)
        row_bytes = eng.pairs * eng.M * (16 if cross else 8)
        chunk = max(group, CHUNK_BYTES // row_bytes // group * group)              # whole columns per chunk
        rows = torch.empty((min(chunk, frames), eng.pairs, eng.M, 2, 2) if cross else (min(chunk, frames), eng.pairs, eng.M, 2),
                           dtype=torch.float32, device=eng.device)

        def store(first, n):
            if cross:
                eng.stft_batch_complex(pcm, first_frame=first, max_frames=n, out=rows)
            else:
                eng.stft_batch(pcm, first_frame=first, max_frames=n, out=rows)
            return rows[:n]

        def terms(r):
            if not cross:
                return r * r
            a_, b_, c_, d_ = r[..., 0, 0], r[..., 0, 1], r[..., 1, 0], r[..., 1, 1]
            return torch.stack([a_ * a_ + b_ * b_, c_ * c_ + d_ * d_, a_ * c_ + b_ * d_, b_ * c_ - a_ * d_], -1)

        def stored_rows_then_torch():
            for first in range(0, frames, chunk):
                n = min(chunk, frames - first)
                x = terms(store(first, n))
                whole = n // group
                j = first // group
                if whole:
                    out[j:j + whole] = x[:whole * group].view(whole, group, *x.shape[1:]).mean(1)
                if n % group:
                    out[j + whole] = x[whole * group:].mean(0)

        def stored_rows_alone():
            for first in range(0, frames, chunk):
                store(first, min(chunk, frames - first))

        call = (lambda e: (lambda: e.csd_batch(pcm, group, out=out))) if cross else (lambda e: (lambda: e.psd_batch(pcm, group, out=out)))
        fused = eng.csd_fused if cross else eng.psd_fused
        legs = {}
        if fused:
            legs["fused"] = call(eng)
            legs["workspace"] = call(split)
        else:
            legs["workspace"] = call(eng)
        legs["stored_rows_then_torch"] = stored_rows_then_torch
        legs["stored_rows_alone"] = stored_rows_alone

        def one_round():
            ms = {}
            for k, run in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                ms[k] = t0.elapsed_time(t1)
            return ms

        t_end = time.perf_counter() + a.settle
        one_round()
        while time.perf_counter() < t_end:
            one_round()
        rounds = [one_round() for _ in range(a.iters)]
        for k in legs:
            rate = np.sort(frames / (np.array([r[k] for r in rounds]) / 1e3))
            q = lambda f: float(rate[min(len(rate) - 1, int(f * len(rate)))])
            print(json.dumps({"case": name, "leg": k, "W": W, "H": H, "channels": ch, "frames": frames, "group": group, "iters": a.iters,
                              "fused": fused, "stft_kernel": eng.info.stft_kernel, "median_frames_per_s": round(q(0.5), 1),
                              "p10_frames_per_s": round(q(0.1), 1), "p90_frames_per_s": round(q(0.9), 1),
                              "min_frames_per_s": round(float(rate[0]), 1), "max_frames_per_s": round(float(rate[-1]), 1),
                              "spread_p10_p90_of_median": round((q(0.9) - q(0.1)) / q(0.5), 4)}), flush=True)
        del pcm, rows, out
        eng.close()
        split.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

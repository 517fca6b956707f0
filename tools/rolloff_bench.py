"""Rates of sgx_rolloff_batch (PCM to the crossings of each frame's cumulative spectrum) against its yardsticks and against what the same
result costs with the entry points the library had before.  Legs, timed interleaved in one process on one device, every round kept:

    rolloff_p1               (a) the call itself at power 2, p = (0.85): rows through the 192 MiB workspace, the kernel over them
    rolloff_p3               (a') the same with three shares (0.85, 0.5, 0.95)
    maxima_k8                (b) sgx_maxima_batch at K = 8 on the same stream: the same route, each row read once as well
    stored_rows_then_torch   (c) sgx_stft_batch in 2 GiB chunks of stored rows; square, torch.cumsum and torch.searchsorted over them
    stored_rows_alone        (d) that row store alone
    rolloff_mags             (e) sgx_rolloff_mags on resident rows (the kernel alone), p = (0.85) ...
    maxima_mags                  ... beside sgx_maxima_mags at K = 8 on the same rows

One JSON line per workload and leg: the median rate, the spread of the rounds (p10 .. p90 and min .. max, as rates); then one line of
ratios of the medians.  The first `--settle` seconds of rounds load the device and are not counted.  Leg (c) finds the bins for one share
and does not gather c[j* - 1], c[j*] and T into records: it is a lower bound on the workaround's cost.

    python tools/rolloff_bench.py [--iters 10] [--settle 3] [--frames 1000000] [--resident 65536] [--case mono ...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {   # name: (W, H, channels)
    "mono": (2048, 256, 1),
    "lr": (2048, 256, 2),
}
CHUNK_BYTES = 2 << 30
POWER = 2
P1 = (0.85,)
P3 = (0.85, 0.5, 0.95)
K = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--settle", type=float, default=3.0, help="seconds of interleaved rounds before the counted ones")
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--resident", type=int, default=65536, help="frames of rows the stage legs run over")
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch = CASES[name]
        frames = a.frames
        eng = SpectrogramEngine(48000.0, window_samples=W, hop_samples=H, channels=ch, device=0)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        out1 = torch.empty((frames, eng.pairs, 2, len(P1), 4), dtype=torch.float32, device=eng.device)
        out3 = torch.empty((frames, eng.pairs, 2, len(P3), 4), dtype=torch.float32, device=eng.device)
        out_max = torch.empty((frames, eng.pairs, 2, K, 4), dtype=torch.float32, device=eng.device)
        row_bytes = eng.pairs * eng.M * 8
        chunk = min(frames, CHUNK_BYTES // row_bytes)
        rows = torch.empty((chunk, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        bins = torch.empty((frames, eng.pairs, 2, len(P1)), dtype=torch.int64, device=eng.device)
        share = torch.tensor(P1, dtype=torch.float32, device=eng.device)
        resident = min(a.resident, chunk)
        res_out = torch.empty((resident, eng.pairs, 2, len(P1), 4), dtype=torch.float32, device=eng.device)
        res_max = torch.empty((resident, eng.pairs, 2, K, 4), dtype=torch.float32, device=eng.device)

        def store(first, n):
            eng.stft_batch(pcm, first_frame=first, max_frames=n, out=rows)
            return rows[:n]

        def stored_rows_then_torch(piece=4096):
            for first in range(0, frames, chunk):
                r = store(first, min(chunk, frames - first))
                for lo in range(0, r.shape[0], piece):                            # (the squares of a whole chunk would double its 2 GiB)
                    m = r[lo:lo + piece]
                    c = (m * m).transpose(2, 3).contiguous().cumsum(-1)           # [piece][pairs][2][M]
                    bins[first + lo:first + lo + m.shape[0]] = torch.searchsorted(c, c[..., -1:] * share)

        def stored_rows_alone():
            for first in range(0, frames, chunk):
                store(first, min(chunk, frames - first))

        legs = {
            "rolloff_p1": lambda: eng.rolloff_batch(pcm, POWER, P1, out=out1),
            "rolloff_p3": lambda: eng.rolloff_batch(pcm, POWER, P3, out=out3),
            "maxima_k8": lambda: eng.maxima_batch(pcm, K, 0.0, out=out_max),
            "stored_rows_then_torch": stored_rows_then_torch,
            "stored_rows_alone": stored_rows_alone,
            "rolloff_mags": lambda: eng.rolloff_mags(rows[:resident], POWER, P1, out=res_out),
            "maxima_mags": lambda: eng.maxima_mags(rows[:resident], K, 0.0, out=res_max),
        }
        work = {leg: resident if leg.endswith("_mags") else frames for leg in legs}

        def one_round():
            ms = {}
            for leg, run in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run()
                t1.record()
                torch.cuda.synchronize()
                ms[leg] = t0.elapsed_time(t1)
            return ms

        t_end = time.perf_counter() + a.settle
        one_round()
        while time.perf_counter() < t_end:
            one_round()
        rounds = [one_round() for _ in range(a.iters)]
        median = {}
        for leg in legs:
            rate = np.sort(work[leg] / (np.array([r[leg] for r in rounds]) / 1e3))
            q = lambda f: float(rate[min(len(rate) - 1, int(f * len(rate)))])
            median[leg] = q(0.5)
            print(json.dumps({"case": name, "leg": leg, "W": W, "H": H, "channels": ch, "frames": work[leg], "power": POWER,
                              "iters": a.iters, "stft_kernel": eng.info.stft_kernel, "median_frames_per_s": round(q(0.5), 1),
                              "p10_frames_per_s": round(q(0.1), 1), "p90_frames_per_s": round(q(0.9), 1),
                              "min_frames_per_s": round(float(rate[0]), 1), "max_frames_per_s": round(float(rate[-1]), 1),
                              "spread_p10_p90_of_median": round((q(0.9) - q(0.1)) / q(0.5), 4)}), flush=True)
        print(json.dumps({"case": name, "ratios_of_medians": {
            "rolloff_p1/maxima_k8": round(median["rolloff_p1"] / median["maxima_k8"], 3),
            "rolloff_p3/maxima_k8": round(median["rolloff_p3"] / median["maxima_k8"], 3),
            "rolloff_p1/stored_rows_then_torch": round(median["rolloff_p1"] / median["stored_rows_then_torch"], 3),
            "rolloff_p1/stored_rows_alone": round(median["rolloff_p1"] / median["stored_rows_alone"], 3),
            "rolloff_mags/maxima_mags": round(median["rolloff_mags"] / median["maxima_mags"], 3)}}), flush=True)
        del pcm, rows, out1, out3, out_max, bins, res_out, res_max
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

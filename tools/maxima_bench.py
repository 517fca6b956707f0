"""Rates of sgx_maxima_batch (PCM to the K strongest spectral maxima per frame, pair and side) against its yardstick and against what the
same result costs with the entry points the library had before.  Legs, timed interleaved in one process on one device, every iteration
kept:

    maxima                   (a) the call itself: rows through the 192 MiB workspace, the selection kernel over them
    psd_group32              (b) sgx_psd_batch at group 32 on the same stream: the same rows route, and each row read once as well
    stored_rows_then_torch   (c) sgx_stft_batch in 2 GiB chunks of stored rows, local-maximum masks and torch.topk over them
    stored_rows_alone        (d) that row store alone
    maxima_mags              (e) sgx_maxima_mags on resident rows (the selection kernel alone) ...
    psd_mags                     ... beside sgx_psd_mags at group 32 on the same rows

One JSON line per workload and leg: the median rate, the spread of the iterations (p10 .. p90 and min .. max, as rates); then one line of
ratios (a)/(b), (a)/(c), (a)/(d) and (e)/psd_mags of the medians.  The first `--settle` seconds of iterations load the device and are
not counted.  Leg (c) returns the same bins and centre values as the call but does not gather the neighbour values: it is a lower bound
on the workaround's cost.

    python tools/maxima_bench.py [--iters 40] [--settle 3] [--k 8] [--frames 1000000] [--resident 65536] [--case mono ...]"""
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
PSD_GROUP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--settle", type=float, default=3.0, help="seconds of interleaved iterations before the counted ones")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--floor", type=float, default=0.0)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--resident", type=int, default=65536, help="frames of rows the stage legs run over")
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch = CASES[name]
        frames, k = a.frames, a.k
        eng = SpectrogramEngine(48000.0, window_samples=W, hop_samples=H, channels=ch, device=0)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        out = torch.empty((frames, eng.pairs, 2, k, 4), dtype=torch.float32, device=eng.device)
        psd = torch.empty((-(-frames // PSD_GROUP), eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        row_bytes = eng.pairs * eng.M * 8
        chunk = min(frames, CHUNK_BYTES // row_bytes)
        rows = torch.empty((chunk, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        top_v = torch.empty((frames, eng.pairs, 2, k), dtype=torch.float32, device=eng.device)
        top_j = torch.empty((frames, eng.pairs, 2, k), dtype=torch.int64, device=eng.device)
        resident = min(a.resident, chunk)
        res_out = torch.empty((resident, eng.pairs, 2, k, 4), dtype=torch.float32, device=eng.device)
        res_psd = torch.empty((-(-resident // PSD_GROUP), eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        floor = a.floor

        def store(first, n):
            eng.stft_batch(pcm, first_frame=first, max_frames=n, out=rows)
            return rows[:n]

        def stored_rows_then_torch(piece=4096):
            for first in range(0, frames, chunk):
                r = store(first, min(chunk, frames - first))
                for lo in range(0, r.shape[0], piece):                            # (the masks of a whole chunk would double its 2 GiB)
                    m = r[lo:lo + piece]
                    c = m[:, :, 1:-1]
                    cand = (c > m[:, :, :-2]) & (c >= m[:, :, 2:]) & (c >= floor)
                    v, j = torch.where(cand, c, torch.zeros((), device=m.device)).transpose(2, 3).topk(k, dim=-1)
                    top_v[first + lo:first + lo + m.shape[0]] = v
                    top_j[first + lo:first + lo + m.shape[0]] = j

        def stored_rows_alone():
            for first in range(0, frames, chunk):
                store(first, min(chunk, frames - first))

        legs = {
            "maxima": lambda: eng.maxima_batch(pcm, k, floor, out=out),
            "psd_group32": lambda: eng.psd_batch(pcm, PSD_GROUP, out=psd),
            "stored_rows_then_torch": stored_rows_then_torch,
            "stored_rows_alone": stored_rows_alone,
            "maxima_mags": lambda: eng.maxima_mags(rows[:resident], k, floor, out=res_out),
            "psd_mags": lambda: eng.psd_mags(rows[:resident], PSD_GROUP, out=res_psd),
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
            print(json.dumps({"case": name, "leg": leg, "W": W, "H": H, "channels": ch, "frames": work[leg], "k": k, "floor": floor,
                              "iters": a.iters, "stft_kernel": eng.info.stft_kernel, "median_frames_per_s": round(q(0.5), 1),
                              "p10_frames_per_s": round(q(0.1), 1), "p90_frames_per_s": round(q(0.9), 1),
                              "min_frames_per_s": round(float(rate[0]), 1), "max_frames_per_s": round(float(rate[-1]), 1),
                              "spread_p10_p90_of_median": round((q(0.9) - q(0.1)) / q(0.5), 4)}), flush=True)
        print(json.dumps({"case": name, "ratios_of_medians": {
            "maxima/psd_group32": round(median["maxima"] / median["psd_group32"], 3),
            "maxima/stored_rows_then_torch": round(median["maxima"] / median["stored_rows_then_torch"], 3),
            "maxima/stored_rows_alone": round(median["maxima"] / median["stored_rows_alone"], 3),
            "maxima_mags/psd_mags": round(median["maxima_mags"] / median["psd_mags"], 3)}}), flush=True)
        del pcm, rows, out, psd, top_v, top_j, res_out, res_psd
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

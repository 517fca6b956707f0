"""Rates of sgx_quantile_batch (PCM to per-bin order statistics over groups of frames) against its yardstick and against what the same
result costs with the entry points the library had before.  Legs, timed interleaved in one process on one device, every iteration kept:

    quantile                 (a) the call itself: rows of whole columns through the 192 MiB workspace, the selection kernel over them
    psd                      (b) sgx_psd_batch at the same group on the same stream: the same rows route, each row read once
    stored_rows_then_torch   (c) sgx_stft_batch in 2 GiB chunks of stored rows, torch.kthvalue (n_q = 1) or torch.sort (n_q > 1) along
                                 the frame axis of every column
    stored_rows_alone        (d) that row store alone
    quantile_mags            (e) sgx_quantile_mags on resident rows (the selection kernel alone, path A) ...
    psd_mags                     ... beside sgx_psd_mags at the same group on the same rows
    quantile_mags_path_b     (f) sgx_quantile_mags on the same rows at a group of kLdsFrames + 1: the column read where it lies

One JSON line per workload and leg: the median rate, the spread of the iterations (p10 .. p90 and min .. max, as rates); then one line of
ratios (a)/(b), (a)/(c), (a)/(d), (e)/psd_mags and (f)/(e) of the medians, and whether (a) beats (c) by more than the two spreads
together.  The first `--settle` seconds of iterations load the device and are not counted.  Rates are frames over event time: no
counters are taken here.

    python tools/quantile_bench.py [--iters 40] [--settle 3] [--group 256] [--frames 1000000] [--resident 65536] [--case mono ...] [--nq 1 ...]"""
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
QUANTILES = {1: (0.5,), 3: (0.1, 0.5, 0.9)}
CHUNK_BYTES = 2 << 30
LDS_FRAMES = 512            # spectrogram_rs_amd/csrc/sgx_quantile.hpp: kLdsFrames
PIECE_COLUMNS = 64          # columns torch reduces at once in leg (c): a sort of a whole chunk would triple its 2 GiB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--settle", type=float, default=3.0, help="seconds of interleaved iterations before the counted ones")
    ap.add_argument("--group", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--resident", type=int, default=65536, help="frames of rows the stage legs run over")
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--nq", action="append", type=int, choices=sorted(QUANTILES))
    a = ap.parse_args()

    import numpy as np
    import torch
    from spectrogram_rs_amd import SpectrogramEngine

    for name in a.case or list(CASES):
        W, H, ch = CASES[name]
        frames, group = a.frames, a.group
        eng = SpectrogramEngine(48000.0, window_samples=W, hop_samples=H, channels=ch, device=0)
        pcm = eng.white_noise(W + (frames - 1) * H, seed=7)
        cols = -(-frames // group)
        row_bytes = eng.pairs * eng.M * 8
        chunk = min(frames, CHUNK_BYTES // row_bytes // group * group)             # whole columns per chunk of stored rows
        rows = torch.empty((chunk, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        psd = torch.empty((cols, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        resident = min(a.resident, chunk) // group * group
        res_psd = torch.empty((resident // group, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
        for nq in a.nq or sorted(QUANTILES):
            q = QUANTILES[nq]
            out = torch.empty((cols, nq, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
            ref = torch.empty_like(out)
            res_out = torch.empty((resident // group, nq, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)
            res_b = torch.empty((-(-resident // (LDS_FRAMES + 1)), nq, eng.pairs, eng.M, 2), dtype=torch.float32, device=eng.device)

            def store(first, n):
                eng.stft_batch(pcm, first_frame=first, max_frames=n, out=rows)
                return rows[:n]

            def reduce_columns(r, dst):
                """whole columns of `group` frames and a short last one, PIECE_COLUMNS at a time"""
                n = r.shape[0]
                for lo in range(0, n, PIECE_COLUMNS * group):
                    m = r[lo:lo + PIECE_COLUMNS * group]
                    whole = m.shape[0] // group
                    parts = [(m[:whole * group].view(whole, group, -1), group)] if whole else []
                    if m.shape[0] % group:
                        parts.append((m[whole * group:].view(1, m.shape[0] % group, -1), m.shape[0] % group))
                    c = lo // group
                    for v, n_j in parts:
                        ranks = [int(np.floor(x * (n_j - 1) + 0.5)) for x in q]
                        if nq == 1:
                            dst[c:c + v.shape[0], 0] = v.kthvalue(ranks[0] + 1, dim=1).values.view(v.shape[0], *dst.shape[2:])
                        else:
                            s = v.sort(dim=1).values
                            for i, k in enumerate(ranks):
                                dst[c:c + v.shape[0], i] = s[:, k].view(v.shape[0], *dst.shape[2:])
                        c += v.shape[0]

            def stored_rows_then_torch():
                for first in range(0, frames, chunk):
                    reduce_columns(store(first, min(chunk, frames - first)), ref[first // group:])

            def stored_rows_alone():
                for first in range(0, frames, chunk):
                    store(first, min(chunk, frames - first))

            legs = {
                "quantile": lambda: eng.quantile_batch(pcm, group, q, out=out),
                "psd": lambda: eng.psd_batch(pcm, group, out=psd),
                "stored_rows_then_torch": stored_rows_then_torch,
                "stored_rows_alone": stored_rows_alone,
                "quantile_mags": lambda: eng.quantile_mags(rows[:resident], group, q, out=res_out),
                "psd_mags": lambda: eng.psd_mags(rows[:resident], group, out=res_psd),
                "quantile_mags_path_b": lambda: eng.quantile_mags(rows[:resident], LDS_FRAMES + 1, q, out=res_b),
            }
            work = {leg: resident if "_mags" in leg else frames for leg in legs}

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
            same = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))   # (noise rows: finite and > 0, torch's order is the key's)
            while time.perf_counter() < t_end:
                one_round()
            rounds = [one_round() for _ in range(a.iters)]
            median, spread = {}, {}
            for leg in legs:
                rate = np.sort(work[leg] / (np.array([r[leg] for r in rounds]) / 1e3))
                at = lambda f: float(rate[min(len(rate) - 1, int(f * len(rate)))])
                median[leg], spread[leg] = at(0.5), (at(0.9) - at(0.1)) / at(0.5)
                print(json.dumps({"case": name, "n_q": nq, "leg": leg, "W": W, "H": H, "channels": ch, "frames": work[leg],
                                  "group": LDS_FRAMES + 1 if leg.endswith("path_b") else group, "iters": a.iters,
                                  "stft_kernel": eng.info.stft_kernel, "median_frames_per_s": round(at(0.5), 1),
                                  "p10_frames_per_s": round(at(0.1), 1), "p90_frames_per_s": round(at(0.9), 1),
                                  "min_frames_per_s": round(float(rate[0]), 1), "max_frames_per_s": round(float(rate[-1]), 1),
                                  "spread_p10_p90_of_median": round(spread[leg], 4)}), flush=True)
            a_c = median["quantile"] / median["stored_rows_then_torch"]
            print(json.dumps({"case": name, "n_q": nq, "call_equals_store_and_reduce_bit_for_bit": same, "ratios_of_medians": {
                "quantile/psd": round(median["quantile"] / median["psd"], 3),
                "quantile/stored_rows_then_torch": round(a_c, 3),
                "quantile/stored_rows_alone": round(median["quantile"] / median["stored_rows_alone"], 3),
                "quantile_mags/psd_mags": round(median["quantile_mags"] / median["psd_mags"], 3),
                "quantile_mags_path_b/quantile_mags": round(median["quantile_mags_path_b"] / median["quantile_mags"], 3)},
                "gate_a_beats_c_by_more_than_both_spreads": bool(a_c - 1.0 > spread["quantile"] + spread["stored_rows_then_torch"])}), flush=True)
            del out, ref, res_out, res_b
        del pcm, rows, psd, res_psd
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The claimed tail of the mono rows launch (csrc/run_claim.hpp) over a grid of static shares and chunk lengths, in ONE process on ONE
device through sgx_set_run_claim: 1e6 frames into each of three output buffers kept alive (the first allocation among them), the
configurations taking turns -- the static split at the head AND the tail of every turn: their difference is the A/A spread the grid is read
against.  Per configuration and buffer: the median launch time over the rounds (each the mean of `launches` back-to-back launches).
usage: tools/k1r_claim_grid.py [--frames N] [--rounds R] [--launches L] [--shares 8,12,14] [--chunks 4,8,16,32]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spectrogram_rs_amd import SpectrogramEngine

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=12)
ap.add_argument("--shares", default="8,12,14")
ap.add_argument("--chunks", default="4,8,16,32")
args = ap.parse_args()
F = args.frames
eng = SpectrogramEngine(48000.0, window_samples=2048, hop_samples=256, channels=1, interp=1, gradient="viridis")
bufs = [torch.empty((F, 1, 2047, 2), dtype=torch.float32, device="cuda") for _ in range(3)]
pcm = eng.white_noise((F - 1) * 256 + 2048)
grid = [(int(s), int(k)) for s in args.shares.split(",") for k in args.chunks.split(",")]
configs = [("static", (16, 0))] + [(f"{s:2d}/16 x {k:2d}", (s, k)) for s, k in grid] + [("static'", (16, 0))]


def timed(out):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.stft_batch(pcm, out=out)
    e0.record()
    for _ in range(args.launches):
        eng.stft_batch(pcm, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.launches


for _ in range(100):      # heat
    eng.stft_batch(pcm, out=bufs[0])
torch.cuda.synchronize()
res = {(name, b): [] for name, _ in configs for b in range(3)}
for _ in range(args.rounds):
    for b, out in enumerate(bufs):
        for name, (s, k) in configs:
            eng.set_run_claim(s, k)
            res[(name, b)].append(timed(out))
eng.set_run_claim(0, 0)
print(f"{F} frames, {args.rounds} rounds of {args.launches} launches; median ms per launch on buffer 0 (first allocation), 1, 2; ratio to static (mean of the three)")
base = [statistics.median(res[("static", b)]) for b in range(3)]
for name, _ in configs:
    med = [statistics.median(res[(name, b)]) for b in range(3)]
    print(f"  {name:12s} " + "  ".join(f"{m:.4f}" for m in med) + f"   {sum(m / a for m, a in zip(med, base)) / 3:.4f}", flush=True)
print("automatic rule:", eng.run_claim(F))

#!/usr/bin/env python3
"""The claimed tail of the mono rows launch (csrc/run_claim.hpp) over a grid of static shares and chunk lengths, in ONE process on ONE
device through sgx_set_run_claim: 1e6 frames into each of three output buffers kept alive (the first allocation among them), the
configurations taking turns -- the static split at the head AND the tail of every turn: their difference is the A/A spread the grid is read
against.  Per configuration and buffer: the median launch time over the rounds (each the mean of `launches` back-to-back launches).
--weights adds every grid point once more under those slot weights (sgx_set_run_weights; the static runs sized by the workgroup's slot on its CU),
--head the configuration at the head and the tail of every turn instead of the static split, --kind and --hop the rows and the hop.
usage: tools/k1r_claim_grid.py [--frames N] [--rounds R] [--launches L] [--shares 8,12,14] [--chunks 4,8,16,32] [--weights 88,80,48,40] [--head 12,8]
       [--kind stft|f16|complex] [--hop H]"""
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
ap.add_argument("--weights", default="", help="slot weights w0,w1,w2,w3: every grid point under equal runs and under these")
ap.add_argument("--head", default="16,0", help="share,chunk of the equal-weights configuration at the head and the tail of every turn")
ap.add_argument("--kind", default="stft", choices=["stft", "f16", "complex"])
ap.add_argument("--hop", type=int, default=256)
args = ap.parse_args()
F = args.frames
EQUAL = (64, 64, 64, 64)
eng = SpectrogramEngine(48000.0, window_samples=2048, hop_samples=args.hop, channels=1, interp=1, gradient="viridis")
DTYPE = {"stft": torch.float32, "f16": torch.float16, "complex": torch.complex64}[args.kind]
bufs = [torch.empty((F, 1, 2047, 2), dtype=DTYPE, device="cuda") for _ in range(3)]
pcm = eng.white_noise((F - 1) * args.hop + 2048)
call = {"stft": eng.stft_batch, "f16": eng.stft_batch_f16, "complex": eng.stft_batch_complex}[args.kind]
grid = [(int(s), int(k)) for s in args.shares.split(",") for k in args.chunks.split(",")]
head = tuple(int(x) for x in args.head.split(","))
head_name = "static" if head == (16, 0) else f"head {head[0]}/16 x {head[1]}"
configs = [(head_name, head, EQUAL)] + [(f"{s:2d}/16 x {k:2d}", (s, k), EQUAL) for s, k in grid]
if args.weights:
    wv = tuple(int(x) for x in args.weights.split(","))
    configs += [(f"{s:2d}/16 x {k:2d} w", (s, k), wv) for s, k in grid]
configs += [(head_name + "'", head, EQUAL)]


def timed(out):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call(pcm, out=out)
    e0.record()
    for _ in range(args.launches):
        call(pcm, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.launches


for _ in range(100):      # heat
    call(pcm, out=bufs[0])
torch.cuda.synchronize()
res = {(name, b): [] for name, _, _ in configs for b in range(3)}
for _ in range(args.rounds):
    for b, out in enumerate(bufs):
        for name, (s, k), w in configs:
            eng.set_run_claim(s, k)
            eng.set_run_weights(w)
            res[(name, b)].append(timed(out))
eng.set_run_claim(0, 0)
eng.set_run_weights(None)
print(f"{args.kind} rows, hop {args.hop}, {F} frames, {args.rounds} rounds of {args.launches} launches" + (f"; w: weights {args.weights}" if args.weights else "")
      + f"; median ms per launch on buffer 0 (first allocation), 1, 2; ratio to {head_name} (mean of the three)")
base = [statistics.median(res[(head_name, b)]) for b in range(3)]
for name, _, _ in configs:
    med = [statistics.median(res[(name, b)]) for b in range(3)]
    print(f"  {name:16s} " + "  ".join(f"{m:.4f}" for m in med) + f"   {sum(m / a for m, a in zip(med, base)) / 3:.4f}", flush=True)
print("automatic rule:", eng.run_claim(F), eng.run_weights(F))

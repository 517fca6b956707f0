#!/usr/bin/env python3
"""Two builds of libsgx.so against each other in ONE process on ONE device, on the SAME output buffers: the mono rows launch (1e6 frames)
into each of three buffers kept alive (the first allocation among them), hot; in every round and on every buffer the builds take turns as
A, B, A' -- A' is a second context of build A, and |A - A'| is the A/A spread the difference is read against.  Both libraries are loaded
with local symbol scope.  Per buffer: the median over the rounds of the mean launch time, the ratio B / A, and whether A - B exceeds twice
the spread.
--claim-b / --weights-b force a split / slot weights on build B's context (sgx_set_run_claim, sgx_set_run_weights), --claim-a a split on A's.
usage: tools/k1r_ab_libs.py <libA.so: the base> <libB.so: the change> [--frames N] [--rounds R] [--launches L] [--kind stft|f16|complex] [--hop H]
       [--claim-a S,K] [--claim-b S,K] [--weights-b w0,w1,w2,w3]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spectrogram_rs_amd import SpectrogramEngine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("lib_a")
ap.add_argument("lib_b")
ap.add_argument("--frames", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=12)
ap.add_argument("--kind", default="stft", choices=["stft", "f16", "complex"], help="float rows (the headline), half rows, complex rows")
ap.add_argument("--hop", type=int, default=256)
ap.add_argument("--claim-a", default="")
ap.add_argument("--claim-b", default="")
ap.add_argument("--weights-b", default="")
args = ap.parse_args()
F = args.frames


def engine_of(path):
    """an engine bound to the library at `path` (local scope: the two builds export the same names)"""
    lib = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, restype, argtypes in _lib.SIGNATURES:
        fn = getattr(lib, name, None)
        if fn is not None:          # (a base build may not export what the change adds)
            fn.restype, fn.argtypes = restype, argtypes
    _lib._lib = lib
    try:
        return SpectrogramEngine(48000.0, window_samples=2048, hop_samples=args.hop, channels=1, interp=1, gradient="viridis")
    finally:
        _lib._lib = None


torch.cuda.init()
DTYPE = {"stft": torch.float32, "f16": torch.float16, "complex": torch.complex64}[args.kind]
bufs = [torch.empty((F, 1, 2047, 2), dtype=DTYPE, device="cuda") for _ in range(3)]
engs = {"A": engine_of(args.lib_a), "B": engine_of(args.lib_b), "A'": engine_of(args.lib_a)}
pcm = engs["A"].white_noise((F - 1) * args.hop + 2048)
if args.claim_a:
    for n in ("A", "A'"):
        engs[n].set_run_claim(*(int(x) for x in args.claim_a.split(",")))
if args.claim_b:
    engs["B"].set_run_claim(*(int(x) for x in args.claim_b.split(",")))
if args.weights_b:
    engs["B"].set_run_weights([int(x) for x in args.weights_b.split(",")])
print("A runs under", engs["A"].run_claim(F), " B under", engs["B"].run_claim(F), engs["B"].run_weights(F) if hasattr(engs["B"]._lib, "sgx_run_weights") else "")


def launch(eng, out):
    return {"stft": eng.stft_batch, "f16": eng.stft_batch_f16, "complex": eng.stft_batch_complex}[args.kind](pcm, out=out)


def timed(eng, out):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch(eng, out)
    e0.record()
    for _ in range(args.launches):
        launch(eng, out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.launches


for _ in range(100):      # heat
    launch(engs["A"], bufs[0])
torch.cuda.synchronize()
sums = {}
for name, eng in engs.items():      # the same bytes from both builds
    launch(eng, bufs[0])
    torch.cuda.synchronize()
    flat = torch.view_as_real(bufs[0]) if args.kind == "complex" else bufs[0]
    sums[name] = int(flat.view(torch.int16 if args.kind == "f16" else torch.int32)[:4096 * 4094].to(torch.int64).sum())
assert len(set(sums.values())) == 1, sums
res = {(n, b): [] for n in engs for b in range(3)}
for _ in range(args.rounds):
    for b, out in enumerate(bufs):
        for n, eng in engs.items():
            res[(n, b)].append(timed(eng, out))
print(f"A = {args.lib_a}   B = {args.lib_b}   {args.kind} rows, hop {args.hop}, {F} frames, {args.rounds} rounds of {args.launches} launches; the rows of both builds sum to the same words")
ok = True
for b in range(3):
    a, bb, a2 = (statistics.median(res[(n, b)]) for n in ("A", "B", "A'"))
    spread = abs(a - a2)
    better = min(a, a2) - bb > 2 * spread
    ok = ok and better
    print(f"  buffer {b}{' (first allocation)' if b == 0 else ''}: A {a:.4f}  A' {a2:.4f}  B {bb:.4f} ms per launch   B / A {bb / a:.4f}   A/A spread {spread:.4f}   "
          f"{'B is faster by more than twice the spread' if better else 'within twice the spread'}", flush=True)
    print("     per round  A " + " ".join(f"{x:.3f}" for x in res[("A", b)]) + "   B " + " ".join(f"{x:.3f}" for x in res[("B", b)]))
print("B faster on every buffer:", ok)

#!/usr/bin/env python3
"""When the workgroups of K1's (l, r) rows launch (csrc/stft4096_wg.hip, the `stereo4096` leg) finish, relative to the last one, and what
every CU slot (block index // CU count) did: tools/k1r_finish.py for the two-channel kernel.  K1 deals equal static runs and has no pool.
SRC=stft4096_wg.hip tools/build_variant.sh <name> -DSGX_STAMPS=2
usage: SGX_LIB=spectrogram_rs_amd/ab/<name>.so tools/k1_finish.py [frames] [launches per buffer]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from spectrogram_rs_amd import SpectrogramEngine, _lib

F = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 5
lib = _lib.load()
fn = lib.sgx_debug_finish
fn.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
eng = SpectrogramEngine(48000.0, window_samples=2048, hop_samples=256, channels=2, interp=1, gradient="viridis")
bufs = [torch.empty((F, 1, 2047, 2), dtype=torch.float32, device="cuda") for _ in range(3)]   # bufs[0]: the process's first allocation
pcm = eng.white_noise((F - 1) * 256 + 2048)
blocks_max = 4 * eng.cu_limit
raw = (C.c_ulonglong * (4 * blocks_max))()
for _ in range(40):          # heat
    eng.stft_batch(pcm, out=bufs[0])
torch.cuda.synchronize()
for bi, out in enumerate(bufs):
    fracs, jobs, ms = [], [], []
    for rep in range(LAUNCHES + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.stft_batch(pcm, out=out)
        e1.record()
        torch.cuda.synchronize()
        assert fn(raw, blocks_max) == 0
        if rep == 0:
            continue         # the first launch on a buffer: not counted
        rec = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).astype(np.int64)
        rec = rec[rec[:, 3] > 0]
        assert (rec[:, 2] == np.arange(len(rec))).all(), "a record that is not this launch's"
        t0, t1 = rec[:, 0].min(), rec[:, 1].max()
        fracs.append((rec[:, 1] - t0) / float(t1 - t0))
        jobs.append(rec[:, 3])
        ms.append(e0.elapsed_time(e1))
    frac, done = np.mean(fracs, axis=0), np.mean(jobs, axis=0)
    idx = np.arange(len(frac))
    d = np.percentile(frac, [10, 30, 50, 70, 90])
    print(f"== buffer {bi}{' (first allocation)' if bi == 0 else ''}: {len(frac)} workgroups, launch {np.median(ms):.4f} ms (median by events); finish / launch duration, mean of "
          f"{LAUNCHES} launches: mean {frac.mean():.4f}  first {frac.min():.4f}  deciles 10/30/50/70/90 " + " ".join(f"{v:.3f}" for v in d))
    for k in range(4):
        sel = np.minimum(idx // eng.cu_limit, 3) == k
        if sel.any():
            print(f"  slot {k}  n {int(sel.sum()):5d}  mean jobs {done[sel].mean():9.2f}  finish mean {frac[sel].mean():.4f}  min {frac[sel].min():.4f}  max {frac[sel].max():.4f}")

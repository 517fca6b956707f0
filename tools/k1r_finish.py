#!/usr/bin/env python3
"""When the workgroups of K1R's mono rows launch (csrc/stft4096_real.hip, the headline) finish, relative to the last one: a diagnostic build
stamps the wall clock (100 MHz, common to all CUs) at the entry and the exit of every workgroup, with the block index and the jobs it did.
SRC=stft4096_real.hip tools/build_variant.sh <name> -DSGX_STAMPS=2   (2: the finish stamps alone, the iteration is the product's; 1: with
the phase stamps of tools/k1r_phases.py, which slow the iteration).
For every output buffer -- the first allocation and two more, all kept alive -- on a hot device: finish time of a workgroup as a fraction of
the launch (first entry to last exit): min, deciles, mean; the same by XCD (block index % 8) and by eighth of the output buffer.
Per slot of the CU (block index // CU count: the n-th workgroup placed on its CU, csrc/run_claim.hpp): the mean jobs done and the mean finish;
under a deep pool in which every slot still claims at the end, jobs of a slot / jobs of all is that slot's rate ratio.
usage: SGX_LIB=spectrogram_rs_amd/ab/<name>.so tools/k1r_finish.py [frames] [launches per buffer] [share,chunk] [w0,w1,w2,w3] [stft|f16|complex] [hop]
(share,chunk: sgx_set_run_claim for the launches, e.g. 12,8 for a claimed tail or 16,0 for the static split; 0,0 or absent: the library's own
rule.  w0..w3: sgx_set_run_weights, 0,0,0,0 or absent: the library's own)"""
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
fn = lib.sgx_debug_finish_r
fn.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
KIND = sys.argv[5] if len(sys.argv) > 5 else "stft"
HOP = int(sys.argv[6]) if len(sys.argv) > 6 else 256
eng = SpectrogramEngine(48000.0, window_samples=2048, hop_samples=HOP, channels=1, interp=1, gradient="viridis")
if len(sys.argv) > 3:
    eng.set_run_claim(*(int(x) for x in sys.argv[3].split(",")))
if len(sys.argv) > 4:
    eng.set_run_weights([int(x) for x in sys.argv[4].split(",")])
print(f"{KIND} rows, hop {HOP}; split (static sixteenths, chunk jobs):", eng.run_claim(F), " weights:", eng.run_weights(F), "(both as a float rows call has them)")
DTYPE = {"stft": torch.float32, "f16": torch.float16, "complex": torch.complex64}[KIND]
bufs = [torch.empty((F, 1, 2047, 2), dtype=DTYPE, device="cuda") for _ in range(3)]   # bufs[0]: the process's first allocation
pcm = eng.white_noise((F - 1) * HOP + 2048)
call = {"stft": eng.stft_batch, "f16": eng.stft_batch_f16, "complex": eng.stft_batch_complex}[KIND]
blocks_max = 4 * eng.cu_limit
raw = (C.c_ulonglong * (4 * blocks_max))()


def line(name, x):
    d = np.percentile(x, [10, 20, 30, 40, 50, 60, 70, 80, 90])
    return f"  {name:22s} n {len(x):5d}  min {x.min():.3f}  deciles " + " ".join(f"{v:.3f}" for v in d) + f"  mean {x.mean():.3f}"


for _ in range(60):          # heat: about 0.2 s of launches before anything is read
    call(pcm, out=bufs[0])
torch.cuda.synchronize()
for bi, out in enumerate(bufs):
    fracs, means, jobs, ms = [], [], [], []
    for rep in range(LAUNCHES + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(pcm, out=out)
        e1.record()
        torch.cuda.synchronize()
        assert fn(raw, blocks_max) == 0
        if rep == 0:
            continue         # the first launch on a buffer: not counted
        rec = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).astype(np.int64)
        rec = rec[rec[:, 3] > 0]
        assert (rec[:, 2] == np.arange(len(rec))).all(), "a record that is not this launch's"
        t0, t1 = rec[:, 0].min(), rec[:, 1].max()
        frac = (rec[:, 1] - t0) / float(t1 - t0)
        fracs.append(frac)
        means.append(frac.mean())
        jobs.append(rec[:, 3])
        ms.append(e0.elapsed_time(e1))
        print(f"buffer {bi} launch {rep}: {e0.elapsed_time(e1):.3f} ms by events, {(t1 - t0) * 1e-5:.3f} ms first entry to last exit, {len(rec)} workgroups, "
              f"jobs {rec[:, 3].min()}..{rec[:, 3].max()} (sum {rec[:, 3].sum()}), entries spread over {(rec[:, 0].max() - t0) * 1e-2:.1f} us, "
              f"mean finish {frac.mean():.4f}, first {frac.min():.4f}")
    frac = np.mean(fracs, axis=0)    # per workgroup, over the launches
    n = len(frac)
    idx = np.arange(n)
    print(f"== buffer {bi}{' (first allocation)' if bi == 0 else ''}: finish time / launch duration, mean of {LAUNCHES} launches per workgroup; mean of the launch means {np.mean(means):.4f}")
    print(line("all", frac))
    for x in range(8):
        print(line(f"XCD {x}", frac[idx % 8 == x]))
    for k in range(8):
        print(line(f"eighth {k} of the rows", frac[(idx * 8) // n == k]))
    done = np.mean(jobs, axis=0)
    print(f"  by slot of the CU ({eng.cu_limit} CUs); launch {np.median(ms):.4f} ms (median by events), first finisher {frac.min():.4f}")
    for k in range(4):
        sel = np.minimum(idx // eng.cu_limit, 3) == k
        if sel.any():
            print(f"  slot {k}  n {int(sel.sum()):5d}  mean jobs {done[sel].mean():9.2f}  / mean of all {done[sel].mean() / done.mean():.4f}  (x 64 = {64 * done[sel].mean() / done.mean():6.2f})"
                  f"  finish mean {frac[sel].mean():.4f}  min {frac[sel].min():.4f}  max {frac[sel].max():.4f}")

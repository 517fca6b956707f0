"""The claimed tail of the mono rows launches (csrc/run_claim.hpp, csrc/stft4096_real.hip): whatever share of the frame pairs is dealt
statically and however long the claimed chunks are, a rows call writes, bit for bit, what the same call writes with the split forced
static -- and nothing else.  One W 2048 mono context at sgx_set_cu_limit(ctx, 1) (four workgroups), hop 256 (the sliding window) and hop
100 (eight columns per pair), 203 frames (a last job without its second frame) and 64, first_frame 0 and 7, float, half and complex
rows; sgx_set_run_claim forces shares 0/16 and 8/16 with chunks of 1 job, 3 jobs, more than the whole pool, exactly the pool, and a third
of the pool (fewer chunks than workgroups: one claims nothing).  Every call goes into a NaN-prefilled payload between guard rows.  The
same launcher writes the rows of every workspace route of such a context, under the same deal: sgx_psd_batch always, and with
SGX_FLAG_NO_FUSED_RENDER sgx_render_batch, sgx_bands_batch, sgx_bands_peak_batch and sgx_fbank_batch; each of these consumers is held to
its own bytes behind the static split in the same way (CONSUMERS).  The
counter's reset: the same call three times back to back, with a call on a second context in between.  At the automatic rule these shapes
run the static split (sgx_run_claim).  No tolerance is involved.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import bounds_arena as ba
import oracle
from spectrogram_rs_amd import SgxError, SpectrogramEngine, _lib
from test_gpu_bounds import Arena, bank_of, dtype_of, elem_of, row_bytes, rows_of, run, words

pytestmark = pytest.mark.gpu

W, SR = 2048, 48000.0
BLOCKS = 4                          # cu limit 1: four workgroups
SHAPES = [(203, 0), (203, 7), (64, 0), (64, 7)]     # (frames of the call, first_frame)
ROWS_KINDS = ["stft", "f16", "complex"]
# the consumers that launch the rows kernel into the workspace: kind -> engine keywords (the default context; one without the fused modes)
CONSUMERS = {"psd_3": {}, "render": dict(fused_render=False), "bands": dict(fused_render=False), "peak_3": dict(fused_render=False),
             "fbank": dict(fused_render=False)}
KINDS = ROWS_KINDS + list(CONSUMERS)
SHARES = [0, 8]
NAN_F16 = 0x7E007E00
PREFILL = {"f32": ba.NAN_WORD, "f16": NAN_F16, "u8": ba.BYTE_FILL * 0x01010101}


def pool_of(n_frames, share):
    """run_claim.hpp: jobs = frame pairs; the static run is floor(floor(jobs share / 16) / workgroups), the pool what is left"""
    jobs = (n_frames + 1) // 2
    return jobs, jobs - BLOCKS * (jobs * share // 16 // BLOCKS)


def chunks_of(n_frames, share):
    jobs, pool = pool_of(n_frames, share)
    third = -(-pool // 3)
    assert pool >= 9 and -(-pool // third) < BLOCKS
    return [1, 3, pool + 5, pool, third]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    yield torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def open_engine(hop, kind="stft"):
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=hop, channels=1, device=0, gradient="viridis", **CONSUMERS.get(kind, {}))
    assert eng.info.stft_kernel == 2 and eng.info.render_path & 8, "the real-input 4096-point kernel must be the one that runs"
    assert eng.psd_fused == 0
    if CONSUMERS.get(kind):     # every consumer of this context takes the rows from the workspace
        assert eng.info.render_path & 1 == 0 and eng.bands_fused == 0 and eng.bands_peak_fused == 0 and bank_of(eng).fused == 0
    eng.set_cu_limit(1)
    return eng


def finite(torch, kind, want):
    if elem_of(kind) == "u8":
        return True
    return not bool(torch.isnan(want.view(torch.float32 if elem_of(kind) == "f32" else torch.float16)).any())


def stream(torch, hop, seed):
    F = 203 + 7
    return torch.from_numpy(oracle.white_noise((F - 1) * hop + W, seed=seed) * np.float32(0.1)).cuda()


def in_arena(torch, eng, kind, dev, first, n):
    arena = Arena(torch, rows_of(kind, n) * row_bytes(eng, kind), row_bytes(eng, kind), False, PREFILL[elem_of(kind)])
    run(eng, kind, dev, first, n, out=arena.payload(dtype_of(torch, kind)).view(-1))
    torch.cuda.synchronize()
    return arena


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", [256, 100])
def test_every_split_writes_the_static_split_s_bytes(torch_cuda, hop, kind):
    torch = torch_cuda
    eng = open_engine(hop, kind)
    dev = stream(torch, hop, 0xC1A1 + hop)
    for n, first in SHAPES:
        assert eng.run_claim(n) == (16, 0), "at the automatic rule a launch this short is the static one"
        eng.set_run_claim(16, 0)
        want = words(torch, run(eng, kind, dev, first, n)).clone()
        assert finite(torch, kind, want)
        for share in SHARES:
            for chunk in chunks_of(n, share):
                eng.set_run_claim(share, chunk)
                assert eng.run_claim(n) == (share, chunk)
                arena = in_arena(torch, eng, kind, dev, first, n)
                what = (hop, kind, n, first, share, chunk)
                assert arena.guards_intact(), (what, "a guard was written")
                assert torch.equal(arena.payload(), want), (what, "differs from the static split", int((arena.payload() != want).sum()),
                                                            int((arena.payload() == ba.as_i32(PREFILL[elem_of(kind)])).sum()))
        eng.set_run_claim(0, 0)
        assert eng.run_claim(n) == (16, 0)
        arena = in_arena(torch, eng, kind, dev, first, n)      # and the automatic rule's launch, the static one, writes them too
        assert arena.guards_intact() and torch.equal(arena.payload(), want), (hop, kind, n, first, "automatic")


@pytest.mark.parametrize("hop", [256, 100])
def test_the_counter_starts_at_zero_in_every_launch(torch_cuda, hop):
    """the same call three times back to back on one context, a call of another context in between: every launch claims from chunk 0.
    The Welch call between the rows calls launches the same kernel into the workspace: one more memset of the one claim counter, on the
    same stream, and its means are those behind the static split"""
    torch = torch_cuda
    eng, other = open_engine(hop), open_engine(hop)
    dev = stream(torch, hop, 0xC1A2 + hop)
    n, first = 203, 7
    eng.set_run_claim(16, 0)
    back_to_back = ROWS_KINDS[:2] + ["psd_3"] + ROWS_KINDS[2:] + ["psd_3"]
    want = {kind: words(torch, run(eng, kind, dev, first, n)).clone() for kind in back_to_back}
    eng.set_run_claim(8, 3)
    other.set_run_claim(0, 1)
    outs = []
    for rep in range(3):        # enqueued back to back: nothing waits between the launches
        for kind in back_to_back:
            outs.append((rep, kind, in_arena_nosync(torch, eng, kind, dev, first, n)))
        if rep == 1:
            outs.append((rep, "other", in_arena_nosync(torch, other, "stft", dev, first, n)))
    torch.cuda.synchronize()
    for rep, kind, arena in outs:
        assert arena.guards_intact(), (hop, rep, kind)
        assert torch.equal(arena.payload(), want["stft" if kind == "other" else kind]), (hop, rep, kind, "differs from the static split")


def in_arena_nosync(torch, eng, kind, dev, first, n):
    arena = Arena(torch, rows_of(kind, n) * row_bytes(eng, kind), row_bytes(eng, kind), False, PREFILL[elem_of(kind)])
    run(eng, kind, dev, first, n, out=arena.payload(dtype_of(torch, kind)).view(-1))
    return arena


def test_the_automatic_rule_and_the_setter_s_arguments(torch_cuda):
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=256, channels=1, device=0, gradient="viridis")
    lib, ctx = eng._lib, eng._ctx
    s, k = C.c_uint32(), C.c_uint32()
    assert eng.run_claim(1_000_000) != (16, 0), "the flagship launch deals its tail in claimed chunks"
    share, chunk = eng.run_claim(1_000_000)
    assert 0 < share < 16 and chunk >= 1
    jobs = 500_000
    assert jobs * share // 16 // (4 * eng.cu_limit) >= 64, "and keeps a long static run"
    for n in (1, 64, 203, 4096, 64 * 4 * eng.cu_limit):
        assert eng.run_claim(n) == (16, 0), n        # a static run under 64 jobs: the static launch
    eng.set_run_claim(16, 0)
    assert eng.run_claim(1_000_000) == (16, 0)
    eng.set_run_claim(4, 16)
    assert eng.run_claim(64) == (4, 16) and eng.run_claim(1_000_000) == (4, 16)
    for bad in ((8, 0), (17, 1), (17, 0), (4, (1 << 20) + 1), (0xFFFFFFFF, 8)):
        assert lib.sgx_set_run_claim(ctx, *bad) == _lib.SGX_ERR_INVALID_ARG and eng.run_claim(64) == (4, 16), bad
        assert b"sgx_set_run_claim" in lib.sgx_last_error(ctx)
    with pytest.raises(SgxError):
        eng.set_run_claim(3, 0)
    eng.set_run_claim(0, 0)
    assert eng.run_claim(64) == (16, 0) and eng.run_claim(1_000_000) == (share, chunk)
    assert lib.sgx_set_run_claim(C.c_void_p(), 8, 8) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_run_claim(C.c_void_p(), 64, C.byref(s), C.byref(k)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_run_claim(ctx, 64, None, C.byref(k)) == _lib.SGX_ERR_INVALID_ARG
    stereo = SpectrogramEngine(SR, window_samples=W, hop_samples=256, channels=2, device=0, gradient="viridis")
    stereo.set_run_claim(8, 8)
    assert stereo.run_claim(1_000_000) == (16, 0), "only the mono rows launches have a claimed tail"

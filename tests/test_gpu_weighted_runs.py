"""The weighted deal of the mono rows launches (csrc/run_claim.hpp, csrc/stft4096_real.hip): whatever weights size the static runs of the
four workgroups of a compute unit, with a small pool behind them or with none, a rows call writes, bit for bit, what the same call writes
with equal static runs -- and nothing else.  One W 2048 mono context, hop 256 (the sliding window) and hop 100, float, half and complex
rows.  At sgx_set_cu_limit(ctx, 1) -- four workgroups, slot = block -- 203 frames (a last job without its second frame) at first_frame 0
and 7 and 64 frames at 7; at a limit of 2, 97 frames (49 jobs in 7 workgroups: a last slot one short) and 203.  Forced weights
(88, 80, 48, 40), (253, 1, 1, 1) and (1, 1, 1, 253) -- the extreme ones leave some workgroups an empty static run, and where the static
share is under one job per unit of weight all of them -- under the splits (15, 1), (15, 3) and (16, 0): no pool, an exact partition.  Every
call goes into a NaN-prefilled payload between guard rows.  The same call three times back to back still holds.  The consumers that launch
the rows kernel into the workspace (tests/test_gpu_claimed_runs.py: CONSUMERS) are held to their own bytes behind the equal static split
in the same way, and on the whole device one sgx_psd_batch call whose range is long enough for the automatic, measured weights equals
the stage over rows of the equal static split.  No tolerance is involved.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import bounds_arena as ba
import oracle
from spectrogram_rs_amd import SgxError, SpectrogramEngine, _lib
from test_gpu_bounds import Arena, bank_of, dtype_of, elem_of, row_bytes, rows_of, run, words
from test_gpu_claimed_runs import CONSUMERS, ROWS_KINDS, finite

pytestmark = pytest.mark.gpu

W, SR = 2048, 48000.0
SHAPES = [(1, 203, 0), (1, 203, 7), (1, 64, 7), (2, 97, 0), (2, 203, 0)]     # (cu limit, frames of the call, first_frame)
KINDS = ROWS_KINDS + list(CONSUMERS)
WEIGHTS = [(88, 80, 48, 40), (253, 1, 1, 1), (1, 1, 1, 253)]
SPLITS = [(15, 1), (15, 3), (16, 0)]
EQUAL = (64, 64, 64, 64)
NAN_F16 = 0x7E007E00
PREFILL = {"f32": ba.NAN_WORD, "f16": NAN_F16, "u8": ba.BYTE_FILL * 0x01010101}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    yield torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def open_engine(hop, channels=1, kind="stft"):
    eng = SpectrogramEngine(SR, window_samples=W, hop_samples=hop, channels=channels, device=0, gradient="viridis", **CONSUMERS.get(kind, {}))
    if channels == 1:
        assert eng.info.stft_kernel == 2 and eng.info.render_path & 8, "the real-input 4096-point kernel must be the one that runs"
    assert eng.psd_fused == 0
    if CONSUMERS.get(kind):     # every consumer of this context takes the rows from the workspace
        assert eng.info.render_path & 1 == 0 and eng.bands_fused == 0 and eng.bands_peak_fused == 0 and bank_of(eng).fused == 0
    return eng


def stream(torch, hop, seed):
    F = 203 + 7
    return torch.from_numpy(oracle.white_noise((F - 1) * hop + W, seed=seed) * np.float32(0.1)).cuda()


def in_arena(torch, eng, kind, dev, first, n, sync=True):
    arena = Arena(torch, rows_of(kind, n) * row_bytes(eng, kind), row_bytes(eng, kind), False, PREFILL[elem_of(kind)])
    run(eng, kind, dev, first, n, out=arena.payload(dtype_of(torch, kind)).view(-1))
    if sync:
        torch.cuda.synchronize()
    return arena


def equal_static(torch, eng, kind, dev, first, n):
    eng.set_run_weights(EQUAL)
    eng.set_run_claim(16, 0)
    want = words(torch, run(eng, kind, dev, first, n)).clone()
    assert finite(torch, kind, want)
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop", [256, 100])
def test_every_weighted_deal_writes_the_equal_static_split_s_bytes(torch_cuda, hop, kind):
    torch = torch_cuda
    eng = open_engine(hop, kind=kind)
    dev = stream(torch, hop, 0x51A7 + hop)
    for limit, n, first in SHAPES:
        eng.set_cu_limit(limit)
        want = equal_static(torch, eng, kind, dev, first, n)
        for w in WEIGHTS:
            eng.set_run_weights(w)
            assert eng.run_weights(n) == w, "forced weights apply at any CU limit"
            for share, chunk in SPLITS:
                eng.set_run_claim(share, chunk)
                assert eng.run_claim(n) == (share, chunk)
                arena = in_arena(torch, eng, kind, dev, first, n)
                what = (hop, kind, limit, n, first, w, share, chunk)
                assert arena.guards_intact(), (what, "a guard was written")
                assert torch.equal(arena.payload(), want), (what, "differs from the equal static split", int((arena.payload() != want).sum()),
                                                            int((arena.payload() == ba.as_i32(PREFILL[elem_of(kind)])).sum()))
        eng.set_run_weights(None)
        eng.set_run_claim(0, 0)
        assert eng.run_weights(n) == EQUAL and eng.run_claim(n) == (16, 0), "at a CU limit and this short the automatic deal is the equal static one"
        arena = in_arena(torch, eng, kind, dev, first, n)
        assert arena.guards_intact() and torch.equal(arena.payload(), want), (hop, kind, limit, n, first, "automatic")


@pytest.mark.parametrize("hop", [256, 100])
def test_the_same_weighted_call_three_times_back_to_back(torch_cuda, hop):
    torch = torch_cuda
    eng = open_engine(hop)
    dev = stream(torch, hop, 0x51A8 + hop)
    eng.set_cu_limit(2)
    n, first = 203, 7
    back_to_back = ROWS_KINDS[:2] + ["psd_3"] + ROWS_KINDS[2:] + ["psd_3"]      # (the Welch call: the same kernel into the workspace, the same counter)
    want = {kind: equal_static(torch, eng, kind, dev, first, n) for kind in back_to_back}
    outs = []
    for w, split in (((88, 80, 48, 40), (15, 3)), ((253, 1, 1, 1), (16, 0)), ((1, 1, 1, 253), (15, 1))):
        eng.set_run_weights(w)
        eng.set_run_claim(*split)
        for rep in range(3):        # enqueued back to back: nothing waits between the launches
            for kind in back_to_back:
                outs.append((w, split, rep, kind, in_arena(torch, eng, kind, dev, first, n, sync=False)))
    torch.cuda.synchronize()
    for w, split, rep, kind, arena in outs:
        assert arena.guards_intact(), (hop, w, split, rep, kind)
        assert torch.equal(arena.payload(), want[kind]), (hop, w, split, rep, kind, "differs from the equal static split")


def test_a_welch_range_under_the_automatic_measured_weights(torch_cuda):
    """The whole device, nothing forced: a mono W 2048, hop 256 context and a call of 2 * (3 * 4 * n_cu) - 3 frames -- 12 n_cu - 1 frame
    pairs, three to a workgroup and four workgroups on every compute unit, the last pair of one frame.  At group 5 the call is one range
    (bounds_arena.welch_ranges), so the rows launch into the workspace is one of that many frames and takes the measured slot weights,
    which ride in the LUT and seed words of the kernel's arguments.  Its means equal the stage over rows of the equal static split."""
    torch = torch_cuda
    eng = open_engine(256)
    n_cu = eng.cu_limit
    assert n_cu == torch.cuda.get_device_properties(0).multi_processor_count
    n, group = 2 * (3 * 4 * n_cu) - 3, 5
    plan = ba.welch_ranges(W, 1, False, n, group, True)
    assert len(plan.ranges) == 1 and plan.ranges[0].pieces == ((0, n, False),), "one rows launch of all the frames"
    auto = eng.run_weights(n)
    assert auto != EQUAL and auto == eng.run_weights(1_000_000), "the measured weights engage for a rows call of the range's size"
    # (a few pairs more than four per compute unit would not do: 4 n_cu + 2 pairs run two to a workgroup in 2 n_cu + 1 workgroups,
    # fewer than three per compute unit, which is the equal deal)
    assert eng.run_weights(2 * 4 * n_cu + 3) == EQUAL
    dev = eng.white_noise((n - 1) * 256 + W, seed=0x51A9)
    got = eng.psd_batch(dev, group)
    eng.set_run_claim(16, 0)
    eng.set_run_weights(EQUAL)
    assert eng.run_weights(n) == EQUAL and eng.run_claim(n) == (16, 0)
    rows = eng.stft_batch(dev)
    want = eng.psd_mags(rows, group)
    assert got.shape == want.shape == (-(-n // group), 1, eng.M, 2)
    assert torch.equal(words(torch, got), words(torch, want)), "the means behind the weighted deal differ from the stage over the equal static split's rows"
    # and the forced equal static split behind the same call
    assert torch.equal(words(torch, eng.psd_batch(dev, group)), words(torch, want))
    eng.close()


def test_the_automatic_weights_and_the_setter_s_arguments(torch_cuda):
    eng = open_engine(256)
    lib, ctx = eng._lib, eng._ctx
    auto = eng.run_weights(1_000_000)
    assert len(auto) == 4 and all(x >= 1 for x in auto) and sum(auto) == 256
    share, chunk = eng.run_claim(1_000_000)
    if auto != EQUAL:
        assert 14 <= share < 16 and chunk >= 1, "the weighted deal keeps a pool of at most 2/16"
    assert eng.run_weights(64) == EQUAL, "fewer workgroups than CU slots: the equal deal"
    assert eng.run_weights(3 * 2 * eng.cu_limit) == EQUAL, "three workgroups per CU: nothing is co-resident the way it was measured"
    eng.set_cu_limit(max(1, eng.cu_limit // 2))
    assert eng.run_weights(1_000_000) == EQUAL, "a CU limit: the equal deal"
    eng.set_cu_limit(0)
    assert eng.run_weights(1_000_000) == auto
    eng.set_run_weights((88, 80, 48, 40))
    assert eng.run_weights(64) == (88, 80, 48, 40) and eng.run_weights(1_000_000) == (88, 80, 48, 40)
    arr = C.c_uint32 * 4
    for bad in ((64, 64, 64, 65), (64, 64, 64, 63), (128, 0, 64, 64), (256, 0, 0, 0), (0xFFFFFF00, 1, 255, 256)):
        assert lib.sgx_set_run_weights(ctx, arr(*bad)) == _lib.SGX_ERR_INVALID_ARG and eng.run_weights(64) == (88, 80, 48, 40), bad
        assert b"sgx_set_run_weights" in lib.sgx_last_error(ctx)
    with pytest.raises(SgxError):
        eng.set_run_weights((1, 2, 3, 4))
    eng.set_run_weights((0, 0, 0, 0))
    assert eng.run_weights(1_000_000) == auto and eng.run_weights(64) == EQUAL
    eng.set_run_weights((1, 1, 1, 253))
    eng.set_run_weights(None)
    assert eng.run_weights(1_000_000) == auto
    assert lib.sgx_set_run_weights(C.c_void_p(), arr(64, 64, 64, 64)) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_run_weights(C.c_void_p(), 64, arr()) == _lib.SGX_ERR_INVALID_ARG
    assert lib.sgx_run_weights(ctx, 64, None) == _lib.SGX_ERR_INVALID_ARG
    stereo = open_engine(256, channels=2)
    stereo.set_run_weights((88, 80, 48, 40))
    assert stereo.run_weights(1_000_000) == EQUAL, "only the mono rows launches deal by slot"

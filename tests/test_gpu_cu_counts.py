"""Every persistent launch at any compute-unit count: bit for bit what it writes at the device's own (tests/cu_counts.py: the case table,
the job splits restated, the branch each (case, limit) takes; tests/test_cu_counts.py proves on the CPU that no case addresses a row
outside its buffers).  One context per case runs every limit of cu_counts.LIMITS through sgx_set_cu_limit; every entry point the case
serves (the Welch calls behind the rows of every forward case among them: cu_counts.welch_kinds), once over the whole range and once
over a sub-range from an odd first_frame, writes into a NaN-prefilled (pixels: 0xA5) payload
between guards and must leave the bytes of the same call at limit 0, no prefill and both guards intact.  The limit-0 rows are held once
to the float64 truth at the project's white-noise bound; after the sweep limit 0 is set again and one call repeated.  The contexts of the
sweep make their first call at limit 0, so their peak partial columns are allocated at full size: test_a_buffer_sized_at_a_low_limit_is_regrown
allocates them at limit 1 on a fresh context first.  No tolerance is involved anywhere else.

SGX_CU_VARIANT=run_split | k16 (with SGX_LIB naming an omit-only variant library, tools/build_variant.sh) turns the file into the
sensitivity check: the rows and complex rows must then differ exactly at the (case, limit) pairs whose table entry gives a workgroup of
that family more than one job, and everything else must still pass.  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

import bounds_arena as ba
import cu_counts as cc
import edge_signals as es
import oracle
from conftest import chirpz_bound, mags_error
from spectrogram_rs_amd import SpectrogramEngine, _lib
import fbank_reference as fr
import psd_reference as pr
from test_gpu_bounds import Arena, bank_of, dtype_of, elem_of, row_bytes, to_dev, words

pytestmark = pytest.mark.gpu

VARIANT = os.environ.get("SGX_CU_VARIANT", "")
assert VARIANT in ("", "run_split", "k16")
AMPLITUDE = np.float32(0.1)        # tests/test_gpu_edges.py: white noise at a tenth of full scale
NAN_F16 = 0x7E007E00               # two quiet half NaNs
PREFILL = {"f32": ba.NAN_WORD, "f16": NAN_F16, "u8": ba.BYTE_FILL * 0x01010101}
FORWARD_KINDS = ["stft", "f16", "complex", "render", "bands", "peak_3", "peak_run"]
PIXEL_FLAGS = {c.name: dict(fused_render=False) for c in cc.TABLE if c.kind == "pixel"}   # STFT, then the pixel stage, on every pixel context


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    yield torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def device_cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def open_case(torch, case, F):
    """the case's context -- kernel and render_path bits asserted first -- and its white-noise stream of F frames"""
    r = cc.route_of(case)
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", **r.engine_kwargs(), **PIXEL_FLAGS.get(case.name, {}))
    info = eng.info
    assert info.stft_kernel == r.kernel, (case.name, info.stft_kernel)
    assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (case.name, info.render_path)
    if r.bands_fused is not None:
        assert eng.bands_fused == r.bands_fused, (case.name, eng.bands_fused)
    assert eng.cu_limit == device_cu(torch), "a fresh context runs at the device's own count"
    return r, eng


def stream(torch, case, r, F):
    N = (F - 1) * r.H + r.W
    pcm = (oracle.white_noise(N * r.channels, seed=0xC0C0 + cc.TABLE.index(case)) * AMPLITUDE).reshape(N, r.channels)
    return pcm, to_dev(torch, r, pcm)


def held_to_the_truth(case, r, pcm, got):
    """the limit-0 rows [F][pairs][M][2] against es.truth_frame at the route's floor and the project's white-noise bound"""
    bound = chirpz_bound(r.W) if r.kernel == 4 else 1.0
    F = got.shape[0]
    truth = {}

    def ref(t, p):
        if (t, p) not in truth:
            truth[(t, p)] = es.truth_frame(es.frame_lr(pcm[t * r.H:t * r.H + r.W], p), r.W)
        return truth[(t, p)]

    worst = 0.0
    for t in range(F):
        for p in range(r.pairs):
            if r.paired:
                q = t ^ 1
                err = es.pair_error(got[t, p], ref(t, p), r.floor, float(np.abs(ref(q, p)).max()) if q < F else 0.0)
            else:
                err = mags_error(got[t, p], ref(t, p), r.floor)
            worst = max(worst, err)
            assert err <= bound, (case.name, t, p, err, "the limit-0 rows miss the float64 truth")
    print(f"CU-TRUTH {case.name} {F} frames worst {worst:.4f} (bound {bound})")


def held_to_the_definition(torch, case, eng, kind, dev, F, ref_words):
    """the limit-0 sums of a bank call on the first, the middle and the last frame against the header's definition over the engine's own
    rows of those frames (tests/fbank_reference.py), bit for bit: the reference of the sweep is itself right"""
    bank, probe = fr.edge_bank(eng.M), [0, F // 2, F - 1]
    if kind == "fbank":
        want = fr.bank_sums(eng.stft_batch(dev, 0, F)[probe].cpu().numpy(), bank, 2)
    else:
        want = fr.cross_sums(torch.view_as_real(eng.stft_batch_complex(dev, 0, F))[probe].cpu().numpy(), bank)
    got = ref_words.view(torch.float32).view(F, eng.pairs, ba.N_BANK_FILTERS, want.shape[-1])[probe].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case.name, kind, "the limit-0 sums differ from the definition")


def held_to_the_welch_definition(torch, case, eng, kind, dev, F, ref_words):
    """the limit-0 means of a Welch call at group 3 on the first, the middle and the last column (the ragged one) against the header's sum
    order over the engine's own rows of those columns (tests/psd_reference.py), bit for bit"""
    cols = -(-F // 3)
    comps = 2 if kind == "psd_3" else 4
    got = ref_words.view(torch.float32).view(cols, eng.pairs, eng.M, comps).cpu().numpy()
    for j in (0, cols // 2, cols - 1):
        n = min(3, F - 3 * j)
        if kind == "psd_3":
            x = pr.psd_terms(eng.stft_batch(dev, 3 * j, n).cpu().numpy())
        else:
            x = pr.csd_terms(torch.view_as_real(eng.stft_batch_complex(dev, 3 * j, n)).cpu().numpy())
        want = pr.welch_mean(x, 3)
        assert want.shape[0] == 1 and np.array_equal(got[j].view(np.uint32), want[0].view(np.uint32)), (case.name, kind, j, "the limit-0 means differ from the definition")


def run_forward(eng, kind, group, dev, first, n, out=None):
    if kind == "stft":
        return eng.stft_batch(dev, first, n, out=out)
    if kind == "f16":
        return eng.stft_batch_f16(dev, first, n, out=out)
    if kind == "complex":
        return eng.stft_batch_complex(dev, first, n, out=out)
    if kind == "render":
        return eng.render_batch(dev, first, n, out=out)
    if kind == "bands":
        return eng.bands_batch(dev, first, n, out=out)
    if kind == "fbank":
        return bank_of(eng).batch(dev, first, n, out=out)
    if kind == "fbank_cross":
        return bank_of(eng).cross_batch(dev, first, n, out=out)
    if kind == "psd_3":
        return eng.psd_batch(dev, group, first, n, out=out)
    if kind == "csd_3":
        return eng.csd_batch(dev, group, first, n, out=out)
    return eng.bands_peak_batch(dev, group, first, n, out=out)


def in_arena(torch, kind, payload_bytes, row_bytes_, call, want, what, expect_same=True):
    """`call(out)` into a prefilled payload between guards; the payload against `want` (flat int32), the prefill and the guards"""
    prefill = PREFILL[elem_of(kind)]
    arena = Arena(torch, payload_bytes, row_bytes_, False, prefill)
    call(arena.payload(dtype_of(torch, kind)))
    torch.cuda.synchronize()
    assert arena.guards_intact(), (what, "a guard was written")
    same = torch.equal(arena.payload(), want)
    if expect_same:
        assert same, (what, "differs from the same call at limit 0",
                      int((arena.payload() != want).sum()), int((arena.payload() == ba.as_i32(prefill)).sum()))
        assert not bool((arena.payload() == ba.as_i32(prefill)).any()), (what, "a payload word still holds the prefill")
    return same


def forward_case(torch, case, dcu):
    F0 = case.frames
    r, eng = open_case(torch, case, F0)
    streams = {}
    ref = {}          # (F, kind, group, first) -> flat int32 of the call at limit 0

    def at(F):
        if F not in streams:
            streams[F] = stream(torch, case, r, F)
        return streams[F]

    peak_fused = eng.bands_peak_fused
    # the filterbank calls of the 4096-point kernels: fbank_reference.edge_bank at power 2, fused wherever bounds_arena.fbank_fused says so
    bank_kinds = list(cc.bank_kinds(r))
    if bank_kinds:
        fb = bank_of(eng)
        assert (fb.fused, fb.cross_fused) == (ba.fbank_fused(r), ba.fbank_fused(r, cross=True)), (case.name, fb.fused, fb.cross_fused)
    # the Welch calls: on the workspace route everywhere, behind the rows whose split is under test
    welch_kinds = list(cc.welch_kinds(r))
    assert eng.psd_fused == 0 and eng.csd_fused == 0
    for limit in cc.LIMITS:
        n_cu = cc.limit_value(limit, dcu)
        eng.set_cu_limit(0 if limit == 0 else n_cu)
        assert eng.cu_limit == n_cu
        F = cc.frames_at(case, limit)
        pcm, dev = at(F)
        family = cc.forward_split(r, n_cu, 0, F)[0]
        predicted = VARIANT == family and cc.more_than_one_job(case, limit, dcu, family)
        differs = False
        for first, n in cc.forward_calls(case, limit):
            groups = {"peak_3": 3, "peak_run": cc.peak_run_group(r, n, n_cu), "psd_3": 3, "csd_3": 3}
            for kind in FORWARD_KINDS + bank_kinds + welch_kinds:
                group = groups.get(kind, 0)
                key = (F, kind, group, first)
                if key not in ref:
                    eng.set_cu_limit(0)
                    ref[key] = words(torch, run_forward(eng, kind, group, dev, first, n)).clone()
                    if kind == "stft" and first == 0:
                        held_to_the_truth(case, r, pcm, ref[key].view(torch.float32).view(n, r.pairs, r.W - 1, 2).cpu().numpy())
                    if kind in bank_kinds and first == 0:
                        held_to_the_definition(torch, case, eng, kind, dev, F, ref[key])
                    if kind in welch_kinds and first == 0:
                        held_to_the_welch_definition(torch, case, eng, kind, dev, F, ref[key])
                    eng.set_cu_limit(0 if limit == 0 else n_cu)
                rb = row_bytes(eng, "bands" if kind.startswith("peak") else kind)
                rows = -(-n // group) if group else n
                what = (case.name, "limit", limit, kind, group, first, n)
                own_rows = kind in ("stft", "complex")
                same = in_arena(torch, kind, rows * rb, rb, lambda out: run_forward(eng, kind, group, dev, first, n, out=out), ref[key], what,
                                expect_same=not (VARIANT and (own_rows or predicted)))
                if own_rows:
                    differs |= not same
        if VARIANT:
            print(f"CU-VARIANT {VARIANT} {case.name} limit {limit}: rows {'differ' if differs else 'identical'}, predicted {'differ' if predicted else 'identical'}")
            assert differs == predicted, (case.name, "limit", limit, "variant", VARIANT, "rows differ" if differs else "rows identical",
                                          "the table predicts", predicted)
    # back at the device's own count: the bytes are those from before (a lowered limit leaves no state behind)
    eng.set_cu_limit(0)
    pcm, dev = at(F0)
    for kind in ("stft", "peak_3"):
        got = words(torch, run_forward(eng, kind, 3, dev, 0, F0))
        assert torch.equal(got, ref[(F0, kind, 3 if kind == "peak_3" else 0, 0)]), (case.name, kind, "after the sweep")
    assert peak_fused == eng.bands_peak_fused
    eng.close()


def pixel_case(torch, case, dcu):
    F = case.frames
    r, eng = open_case(torch, case, F)
    assert eng.info.render_path & 1 == 0 and eng.bands_fused == 0, (case.name, "the two-kernel pixel stage")
    pcm, dev = stream(torch, case, r, F)
    mags = eng.stft_batch(dev)
    held_to_the_truth(case, r, pcm, mags.cpu().numpy())
    cols = mags.reshape(-1, eng.M, 2).contiguous()
    ends = eng.bin_edges()
    ranges = np.stack([ends[:-1], ends[1:]], 1)
    bands = eng.magnitude_in(cols, ranges).contiguous()
    R = eng.R
    calls = {   # kind -> (element kind, bytes per column, call(first column, out))
        "render": ("render", lambda first, out: eng.render_batch(dev, first, None, out=out), r.pairs * R * 4, r.pairs),
        "bands": ("bands", lambda first, out: eng.bands_batch(dev, first, None, out=out), r.pairs * R * 8, r.pairs),
        "render_mags": ("render_mags", lambda first, out: eng.render_mags(cols[first:], out=out), R * 4, 1),
        "magnitude_in": ("magnitude_in", lambda first, out: eng.magnitude_in(cols[first:], ranges, out=out), R * 8, 1),
        "render_bands": ("render_bands", lambda first, out: eng.render_bands(bands[first:], out=out), R * 4, 1),
    }
    ref = {}
    n_all = {1: F * r.pairs, r.pairs: F}
    for limit in cc.LIMITS:
        n_cu = cc.limit_value(limit, dcu)
        eng.set_cu_limit(0 if limit == 0 else n_cu)
        assert eng.cu_limit == n_cu
        for name, (kind, call, rb, unit) in calls.items():
            for first in (0, case.first):
                if (name, first) not in ref:
                    assert limit == 0
                    ref[(name, first)] = words(torch, call(first, None)).clone()
                n = n_all[unit] - first
                # (a variant library omits work in the TRANSFORM render_batch and bands_batch run first: the forward cases hold that; here the
                # entry points of the pixel stage alone must still pass)
                in_arena(torch, kind, n * rb, rb, lambda out: call(first, out), ref[(name, first)], (case.name, "limit", limit, name, first),
                         expect_same=not (VARIANT and name in ("render", "bands")))
    eng.set_cu_limit(0)
    assert torch.equal(words(torch, calls["render_mags"][1](0, None)), ref[("render_mags", 0)]), (case.name, "after the sweep")
    # the oracle's pixels of the limit-0 rows: the reference of the sweep is itself right
    from spectrogram_rs_amd import builtin_gradient
    want = oracle.render_columns(cols[:3].cpu().numpy(), eng.info.sample_rate_u32, builtin_gradient("viridis"), R=R)
    assert np.array_equal(ref[("render_mags", 0)].view(torch.uint8).view(-1, R, 4)[:3].cpu().numpy(), want)
    eng.close()


def inverse_case(torch, case, dcu):
    F = case.frames
    r, eng = open_case(torch, case, F)
    assert eng.istft_supported() == 1
    pcm, dev = stream(torch, case, r, F)
    N, Cn = pcm.shape
    spec = torch.view_as_real(eng.stft_batch_complex(dev)).contiguous()
    held_to_the_truth(case, r, pcm, eng.stft_batch(dev).cpu().numpy())
    ref = {}
    for limit in cc.LIMITS:
        n_cu = cc.limit_value(limit, dcu)
        eng.set_cu_limit(0 if limit == 0 else n_cu)
        assert eng.cu_limit == n_cu
        for first in (0, case.first):
            if first not in ref:
                assert limit == 0
                ref[first] = words(torch, eng.istft_batch(spec, first_sample=first)).clone()
            n = N - first
            in_arena(torch, "istft", n * Cn * 4, Cn * 4, lambda out: eng.istft_batch(spec, first_sample=first, out=out), ref[first],
                     (case.name, "limit", limit, "istft", first))
    eng.set_cu_limit(0)
    assert torch.equal(words(torch, eng.istft_batch(spec)), ref[0]), (case.name, "after the sweep")
    eng.close()


@pytest.mark.parametrize("case", cc.TABLE, ids=lambda c: c.name)
def test_every_limit_writes_the_bytes_of_the_devices_own_count(torch_cuda, case):
    dcu = device_cu(torch_cuda)
    {"forward": forward_case, "pixel": pixel_case, "inverse": inverse_case}[case.kind](torch_cuda, case, dcu)


def test_the_table_reaches_every_branch(torch_cuda):
    dcu = device_cu(torch_cuda)
    reached = {}
    for case in cc.TABLE:
        for limit in cc.LIMITS:
            for b in cc.branches(case, limit, dcu):
                reached.setdefault(b, []).append((case.name, limit))
    for b in cc.REQUIRED_BRANCHES:
        print(f"CU-BRANCH {b}: {len(reached.get(b, []))} (case, limit) pairs, e.g. {reached.get(b, [None])[0]}")
    assert not set(cc.REQUIRED_BRANCHES) - set(reached), sorted(set(cc.REQUIRED_BRANCHES) - set(reached))
    # the fused bank call of the real-input kernel meets a last job of one frame behind other jobs of its run
    banks = cc.bank_cases_with_a_last_job_of_one_frame(dcu)
    print(f"CU-BRANCH the fused bank kinds at '{cc.LAST_JOB_ONE_FRAME}': {banks}")
    assert {"k1r_h256", "k1r_h100", "k1r_h256_align4"} == {name for name, _ in banks}
    if VARIANT:   # the references of the sensitivity check are themselves untouched by the variant
        assert cc.references_have_one_job(dcu, VARIANT)


@pytest.mark.parametrize("name", ["k1r_h256", "k1_lr_h256", "k1_ch4"])
def test_a_buffer_sized_at_a_low_limit_is_regrown(torch_cuda, name):
    """The one buffer the context sizes by the count, the fused peak route's partial columns: a fresh context makes its FIRST peak call at
    limit 1 (partials of 4 workgroups), its second at limit 0, where 38 or 75 workgroups write theirs; both against the limit-0 columns of
    another context that never saw a lower limit.  A low limit on a context that allocated at the full count would not exercise grow()."""
    torch = torch_cuda
    case = cc.CASE[name]
    r, ref_eng = open_case(torch, case, case.frames)
    assert ref_eng.bands_peak_fused == 1
    _, dev = stream(torch, case, r, case.frames)
    want = words(torch, ref_eng.bands_peak_batch(dev, 3)).clone()
    ref_eng.close()
    _, eng = open_case(torch, case, case.frames)
    rb = row_bytes(eng, "bands")
    for limit in (1, 0, 2, 0):
        eng.set_cu_limit(limit)
        in_arena(torch, "bands", -(-case.frames // 3) * rb, rb, lambda out: eng.bands_peak_batch(dev, 3, out=out), want, (name, "limit", limit),
                 expect_same=not VARIANT)   # (a variant library drops frames at limits 1 and 2: the guards are still held)
    eng.close()


def test_the_limit_contract(torch_cuda):
    import ctypes as C
    dcu = device_cu(torch_cuda)
    eng = SpectrogramEngine(es.SR, device=0, window_samples=2048, hop_samples=256, channels=1)
    lib, ctx = eng._lib, eng._ctx
    assert lib.sgx_cu_limit(ctx) == dcu
    for n in (1, 7, dcu - 1, dcu):
        assert lib.sgx_set_cu_limit(ctx, n) == _lib.SGX_OK and lib.sgx_cu_limit(ctx) == n
    assert lib.sgx_set_cu_limit(ctx, 5) == _lib.SGX_OK
    for n in (dcu + 1, 2 * dcu, 0xFFFFFFFF):
        assert lib.sgx_set_cu_limit(ctx, n) == _lib.SGX_ERR_INVALID_ARG and lib.sgx_cu_limit(ctx) == 5, n
        assert b"sgx_set_cu_limit" in lib.sgx_last_error(ctx)
    with pytest.raises(_lib.SgxError):
        eng.set_cu_limit(dcu + 1)
    assert eng.cu_limit == 5
    assert lib.sgx_set_cu_limit(ctx, 0) == _lib.SGX_OK and lib.sgx_cu_limit(ctx) == dcu
    assert lib.sgx_set_cu_limit(C.c_void_p(), 1) == _lib.SGX_ERR_INVALID_ARG and lib.sgx_cu_limit(C.c_void_p()) == 0
    assert eng.info.struct_size == 64      # sgx_info keeps its 64 bytes
    eng.close()

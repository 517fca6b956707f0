"""Every transform family and every entry point at 6, 12 and 64 channels and at sgx_create's cap of 32 768 (tests/channel_counts.py: the case
table, the streams and the labelling of the cap rows), all through the C ABI.  Per row: the kernel and render_path bits it pins; every
frame and pair of sgx_stft_batch and sgx_stft_batch_complex against the float64 truth at the project's own white-noise bounds (one
CHANNEL-RATIO line per case); the half rows, pixels, bands, peak columns, filterbank and cross sums bit for bit against the stage entry
points on the engine's own rows, fused and (at W 2048) two-kernel, the Welch means also against the header's sum order
(tests/psd_reference.py) over those rows; sub-ranges; the inverse against include/sgx.h's definition, split at an
odd sample and into an 8-mod-16 aligned buffer; a stream of identical pairs, whose every pair must give the bytes of pair 0 (the 4096-point
family: also those of a two-channel context); the 6-channel rows of the persistent kernels at compute-unit limits around their pair count;
sgx_process_one, the noise generator and sgx_create's refusals at odd and too large counts.

The cap rows are compared on the device in chunks of pairs: every one of the 16 384 rows of every frame is held to the truth of its
label.  The 2048- and 8192-point cap rows leave out the complex rows and the filterbank sums (channel_counts.Case.complex_and_banks), and
with them the inverse.  Run with -m gpu on an MI355X."""
import contextlib
import time

import numpy as np
import pytest

import bounds_arena as ba
import channel_counts as cn
import edge_signals as es
import oracle
import psd_reference as pr
from conftest import mags_error
from test_gpu_bands import two_call
from test_gpu_bounds import words
from test_gpu_complex import complex_error, noise_bound, truth_complex
from test_gpu_istft import DEFINITION_TOL, definition
from test_gpu_large import LARGE_BOUND
from test_gpu_peak import amax_groups, same

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cn.TABLE]
CAP_NAMES = [c.name for c in cn.CAP_ROWS]
CAP_CHUNK = 1024            # pairs per comparison on the device
_cache = {}
_wall = {}
assert cn.LARGE_BOUND == LARGE_BOUND["default"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    yield torch
    torch.cuda.synchronize()
    _cache.clear()
    torch.cuda.empty_cache()


class timed:
    """wall time per case, summed over its tests (the CHANNEL-TIME lines of test_wall_times)"""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        _wall[self.name] = _wall.get(self.name, 0.0) + time.perf_counter() - self.t0


def engine(c, **extra):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(es.SR, device=0, gradient="viridis", **c.engine_kwargs(**extra))


def to_dev(torch, pcm, offset_floats=0):
    """the stream on the device, `offset_floats` floats past a 16-byte boundary"""
    flat = torch.from_numpy(np.ascontiguousarray(pcm, np.float32).reshape(-1))
    buf = torch.empty(flat.numel() + 4, dtype=torch.float32, device="cuda")
    lead = (-(buf.data_ptr() // 4) % 4 + offset_floats) % 4
    dev = buf[lead:lead + flat.numel()]
    dev.copy_(flat)
    assert dev.data_ptr() % 16 == 4 * offset_floats
    return dev


class State:
    """a case's stream, context and full rows, built once"""

    def __init__(self, torch, c):
        self.c = c
        self.pcm = cn.build_stream(c)
        self.eng = engine(c)
        self.dev = to_dev(torch, self.pcm)
        if c.cap:
            self.pcm = None     # (a cap row's stream is its labelled base pairs: channel_counts.base_pairs)
        self.rows = self.eng.stft_batch(self.dev)
        self.cx = self.eng.stft_batch_complex(self.dev) if c.complex_and_banks else None
        torch.cuda.synchronize()


def case(torch, name):
    if name not in _cache:
        with timed(torch, name):
            _cache[name] = State(torch, cn.CASE[name])
    return _cache[name]


# ---- 1. the route ------------------------------------------------------------------------------------------------------------------------
def check_route(s):
    c, r, eng = s.c, s.c.route, s.eng
    info = eng.info
    assert (eng.channels, eng.pairs) == (c.channels, c.pairs)
    assert info.stft_kernel == r.kernel, (c.name, info.stft_kernel)
    assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (c.name, info.render_path)
    assert eng.bands_fused == c.bands_fused, (c.name, eng.bands_fused)
    assert eng.bands_peak_fused == c.bank_fused, (c.name, eng.bands_peak_fused)
    assert eng.istft_supported() == (0 if r.kernel == 11 else 1)
    assert tuple(s.rows.shape) == (c.frames, c.pairs, c.W - 1, 2)


# ---- 2. the truth ------------------------------------------------------------------------------------------------------------------------
def check_truth(torch, s):
    c, r = s.c, s.c.route
    if c.cap:
        return check_truth_cap(torch, s)
    got = s.rows.cpu().numpy()
    assert np.isfinite(got).all(), (c.name, "a row holds a NaN or an infinity")
    truth = cn.truth_rows(c, s.pcm)
    worst, where = 0.0, None
    for t in range(c.frames):
        for p in range(c.pairs):
            err = mags_error(got[t, p], truth[t, p], r.floor)
            if not err <= worst:      # (a NaN ratio is the worst, not skipped)
                worst, where = err, (t, p)
    print(f"CHANNEL-RATIO {c.name} worst {worst:.4f} at {where} (bound {c.bound})")
    assert worst <= c.bound, (c.name, where, worst)
    cx = s.cx.cpu().numpy()
    assert cx.dtype == np.complex64 and cx.shape == got.shape
    assert np.isfinite(cx).all(), (c.name, "a complex row holds a NaN or an infinity")
    cworst, cwhere, cbound = 0.0, None, noise_bound(r)
    for t in range(c.frames):
        for p in range(c.pairs):
            ref = truth_complex(es.frame_lr(cn.frame_of(c, s.pcm, t), p), c.W)
            err = complex_error(cx[t, p], ref, r.floor, float(np.abs(ref).max()))
            if not err <= cworst:
                cworst, cwhere = err, (t, p)
    print(f"CHANNEL-COMPLEX-RATIO {c.name} worst {cworst:.4f} at {cwhere} (bound {cbound})")
    assert cworst <= cbound, (c.name, cwhere, cworst)
    assert cbound == c.bound or r.kernel == 11


def check_truth_cap(torch, s):
    """every one of the 16 384 rows of every frame against the truth of its label, on the device in chunks of CAP_CHUNK pairs"""
    c, r = s.c, s.c.route
    lab = torch.from_numpy(cn.labels(c.pairs).copy()).cuda()
    truth = torch.from_numpy(cn.truth_labels(c)).cuda()             # [frames][labels][M][2] float64
    worst, where = 0.0, None
    for p0 in range(0, c.pairs, CAP_CHUNK):
        ratio = cn.device_ratio(torch, s.rows[:, p0:p0 + CAP_CHUNK], truth[:, lab[p0:p0 + CAP_CHUNK]], r.floor)
        assert bool(torch.isfinite(ratio).all())
        m = float(ratio.max())
        if m > worst:
            t, p = divmod(int(ratio.argmax()), ratio.shape[1])
            worst, where = m, (t, p0 + p)
    print(f"CHANNEL-RATIO {c.name} worst {worst:.4f} at {where} (bound {c.bound}), {c.frames * c.pairs} rows each against its label's truth")
    assert worst <= c.bound, (c.name, where, worst)
    del truth
    if not c.complex_and_banks:
        return
    base = cn.base_pairs(c)
    ctruth = torch.from_numpy(np.stack([np.stack([truth_complex(base[k, t * c.H:t * c.H + c.W], c.W) for k in range(cn.N_LABELS)])
                                        for t in range(c.frames)])).cuda()
    cworst, cwhere = 0.0, None
    for p0 in range(0, c.pairs, CAP_CHUNK):
        ratio = cn.device_complex_ratio(torch, s.cx[:, p0:p0 + CAP_CHUNK], ctruth[:, lab[p0:p0 + CAP_CHUNK]], r.floor)
        assert bool(torch.isfinite(ratio).all())
        m = float(ratio.max())
        if m > cworst:
            t, p = divmod(int(ratio.argmax()), ratio.shape[1])
            cworst, cwhere = m, (t, p0 + p)
    print(f"CHANNEL-COMPLEX-RATIO {c.name} worst {cworst:.4f} at {cwhere} (bound {noise_bound(r)})")
    assert cworst <= noise_bound(r), (c.name, cwhere, cworst)


# ---- 3. the derived outputs ------------------------------------------------------------------------------------------------------------
def peak_groups(frames):
    return sorted({1, 2, 4, frames})


@contextlib.contextmanager
def mel_banks(eng, powers=(2, 1)):
    """power -> a 128-filter mel bank on `eng`, destroyed on the way out"""
    fbs = {power: eng.mel_filterbank(128, power=power) for power in powers}
    try:
        yield fbs
    finally:
        for fb in fbs.values():
            fb.close()


CAP_BINS = 8                # bins per row the host reference of the Welch means takes at the cap rows


def check_welch(torch, s, eng, dev, rows, cx, first=0, count=None):
    """sgx_psd_batch (and, where the case runs complex rows, sgx_csd_batch) over frames [first, first + count) of the stream against the
    stage over the same frames of the engine's own rows, bit for bit on the device, and both against the header's sum order
    (tests/psd_reference.py) over those rows: on all bins, at the cap rows on every stride-th.  The groups are those of the peak columns;
    at the cap one column of all frames and group 2.  No context runs a fused mode: the rows go through the workspace, which at 32 768
    channels holds fewer rows than a block of 32 and its partial, or none (bounds_arena.welch_ranges: a frame per piece)."""
    c = s.c
    assert eng.psd_fused == 0 and eng.csd_fused == 0
    end = c.frames if count is None else min(c.frames, first + count)
    n = end - first
    groups = [ba.WELCH_MAX, 2] if c.cap else peak_groups(n)
    stride = max(1, eng.M // CAP_BINS) if c.cap else 1
    kinds = [("psd", rows, eng.psd_batch, eng.psd_mags, pr.psd_terms, 2)]
    if cx is not None:
        kinds.append(("csd", torch.view_as_real(cx), eng.csd_batch, eng.csd_spec, pr.csd_terms, 4))
    for kind, own, batch, stage, terms, comps in kinds:
        x = terms(own[first:end][:, :, ::stride].cpu().numpy())
        for group in groups:
            assert eng.info.mags_bytes_per_frame == ba.mags_bytes_per_frame(c.W, c.pairs)      # (what the model counts the rows by)
            got = batch(dev, group, first_frame=first, max_frames=count)
            assert tuple(got.shape) == (-(-n // min(group, n)), c.pairs, eng.M, comps), (c.name, kind, group, first, count)
            staged = stage(own[first:end].contiguous(), group)
            assert torch.equal(words(torch, got), words(torch, staged)), (c.name, kind, "batch and stage, group", group, first, count)
            want = pr.welch_mean(x, group)
            assert np.array_equal(got[:, :, ::stride].cpu().numpy().view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)), \
                (c.name, kind, "not the definition's bits, group", group, first, count)
            del got, staged


def check_derived(torch, s, eng=None, fused=True):
    """the outputs of `eng` (default the case's own context) against the stage entry points on its own rows"""
    c = s.c
    dev = s.dev
    own = eng is None
    eng = s.eng if own else eng
    rows = s.rows if own else eng.stft_batch(dev)
    if not own:   # the two-kernel context's rows are those of the fused one
        assert torch.equal(words(torch, rows), words(torch, s.rows)), (c.name, "rows of the two-kernel context")
    cols = rows.reshape(-1, eng.M, 2)
    assert torch.equal(eng.stft_batch_f16(dev), rows.half()), (c.name, "half rows")
    px = eng.render_batch(dev)
    assert tuple(px.shape) == (c.frames, c.pairs, eng.R, 4)
    assert torch.equal(px.reshape(-1, eng.R, 4), eng.render_mags(cols)), (c.name, "pixels")
    assert eng.bands_fused == (c.bands_fused if fused else 0), (c.name, eng.bands_fused)
    assert eng.bands_peak_fused == (c.bank_fused if fused else 0), (c.name, eng.bands_peak_fused)
    bands = eng.bands_batch(dev)
    mags, ref = two_call(eng, dev)
    assert torch.equal(words(torch, mags), words(torch, rows))
    assert tuple(bands.shape) == (c.frames, c.pairs, eng.R, 2)
    assert torch.equal(words(torch, bands), words(torch, ref)), (c.name, "bands")
    for group in peak_groups(c.frames):
        peak = eng.bands_peak_batch(dev, group)
        assert tuple(peak.shape) == (-(-c.frames // group), c.pairs, eng.R, 2)
        assert same(peak, amax_groups(bands, group)), (c.name, "peak columns, group", group)
    if not c.complex_and_banks:
        check_welch(torch, s, eng, dev, rows, None)
        return
    cx = s.cx if own else eng.stft_batch_complex(dev)
    if not own:
        assert torch.equal(words(torch, cx), words(torch, s.cx)), (c.name, "complex rows of the two-kernel context")
    check_welch(torch, s, eng, dev, rows, cx)
    with mel_banks(eng) as fbs:
        for power, fb in fbs.items():
            assert fb.n_filters == 128
            assert fb.fused == (c.bank_fused if fused else 0), (c.name, power, fb.fused)
            got = fb.batch(dev)
            assert tuple(got.shape) == (c.frames, c.pairs, 128, 2)
            assert torch.equal(words(torch, got), words(torch, fb.apply(cols))), (c.name, "filterbank sums, power", power)
            if power == 2:
                assert fb.cross_fused == (c.bank_fused if fused else 0), (c.name, fb.cross_fused)
                cross = fb.cross_batch(dev)
                assert tuple(cross.shape) == (c.frames, c.pairs, 128, 4)
                staged = fb.cross_apply(torch.view_as_real(cx).reshape(-1, eng.M, 2, 2))
                assert torch.equal(words(torch, cross), words(torch, staged)), (c.name, "cross sums")


# ---- 4. sub-ranges -------------------------------------------------------------------------------------------------------------------------
def check_sub_ranges(torch, s):
    c, eng, dev, F = s.c, s.eng, s.dev, s.c.frames
    if F == 1:    # (the one-frame cap rows have no sub-range: frame 0 alone is the full call)
        return
    calls = [(f, n) for f, n in ((1, 1), (1, 3), (2, 1), (2, 3), (F - 1, 1), (0, 1)) if f < F]
    bands = eng.bands_batch(dev)
    for first, count in dict.fromkeys(calls):
        end = min(F, first + count)
        part = eng.stft_batch(dev, first_frame=first, max_frames=count)
        assert torch.equal(words(torch, part), words(torch, s.rows[first:end])), (c.name, "rows", first, count)
        part = eng.bands_batch(dev, first_frame=first, max_frames=count)
        assert torch.equal(words(torch, part), words(torch, bands[first:end])), (c.name, "bands", first, count)
        if s.cx is not None:
            part = eng.stft_batch_complex(dev, first_frame=first, max_frames=count)
            assert torch.equal(words(torch, part), words(torch, s.cx[first:end])), (c.name, "complex rows", first, count)
        check_welch(torch, s, eng, dev, s.rows, s.cx, first, count)     # (the columns counted from the sub-range's own first frame)


# ---- 5. the inverse ----------------------------------------------------------------------------------------------------------------------
def check_inverse(torch, s):
    c, eng = s.c, s.eng
    N = c.samples
    whole = eng.istft_batch(s.cx)
    assert tuple(whole.shape) == (N, c.channels)
    ref, env = definition(s.cx.cpu().numpy(), c.W, c.H, eng.window(), c.channels)
    worst = cn.inverse_ratio(torch, whole.cpu().numpy(), ref, env, c.W, c.H, eng.window(), DEFINITION_TOL, device="cuda")
    print(f"CHANNEL-INVERSE {c.name} worst {worst:.4f} of the definition bound")
    assert worst <= 1.0, (c.name, worst)
    cut = (N // 2) | 1
    parts = torch.cat([eng.istft_batch(s.cx, first_sample=0, max_samples=cut), eng.istft_batch(s.cx, first_sample=cut)], 0)
    assert torch.equal(words(torch, parts), words(torch, whole)), (c.name, "split at the odd sample", cut)
    buf = torch.empty(N * c.channels + 4, dtype=torch.float32, device="cuda")
    lead = (-(buf.data_ptr() // 4) % 4 + 2) % 4
    out = buf[lead:lead + N * c.channels]
    assert out.data_ptr() % 16 == 8
    got = eng.istft_batch(s.cx, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(words(torch, got), words(torch, whole)), (c.name, "an output buffer at 8 modulo 16 bytes")


# ---- 6. identical pairs ------------------------------------------------------------------------------------------------------------------
def all_pairs_are_pair_0(torch, t):
    """[F][pairs][...]: every pair's bytes those of pair 0"""
    v = torch.view_as_real(t) if t.is_complex() else t
    v = v.contiguous().view(torch.int32)
    return bool((v == v[:, :1]).all())


def check_identical_pairs(torch, s):
    from spectrogram_rs_amd import SpectrogramEngine
    c, eng = s.c, s.eng
    pcm = cn.identical_stream(c)
    dev = to_dev(torch, pcm)
    def outputs(e, d):
        outs = {"rows": e.stft_batch(d), "bands": e.bands_batch(d), "Welch means": e.psd_batch(d, 2)}
        if c.complex_and_banks:
            outs["complex rows"] = e.stft_batch_complex(d)
            outs["Welch cross means"] = e.csd_batch(d, 2)
            with mel_banks(e, powers=(2,)) as fbs:
                outs["filterbank sums"] = fbs[2].batch(d)
        return outs

    outs = outputs(eng, dev)
    for what, t in outs.items():
        # (bit comparisons take a NaN for a NaN: the rows of this stream are held finite here, those of the case's own stream to the truth)
        assert bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()), (c.name, what, "not finite")
        assert all_pairs_are_pair_0(torch, t), (c.name, what, "a pair differs from pair 0 on the same samples")
    if c.route.kernel != 2:
        return
    # the 4096-point family runs the two-channel kernel on a plane: the bytes of a two-channel context fed that (l, r)
    two = SpectrogramEngine(es.SR, device=0, gradient="viridis", **c.engine_kwargs(channels=2))
    assert two.info.stft_kernel == 2
    for what, t in outputs(two, to_dev(torch, pcm[:, :2])).items():
        assert torch.equal(words(torch, outs[what][:, :1]), words(torch, t)), (c.name, what, "differs from a two-channel context")
    two.close()


# ---- the tests of the 6-, 12- and 64-channel rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_route(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_route(s)


@pytest.mark.parametrize("name", NAMES)
def test_every_frame_and_pair_against_the_truth(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_truth(torch_cuda, s)


@pytest.mark.parametrize("name", NAMES)
def test_derived_outputs_are_those_of_the_rows(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_derived(torch_cuda, s)
        if s.c.W == 2048:
            split = engine(s.c, fused_render=False)
            assert split.info.render_path & 1 == 0
            check_derived(torch_cuda, s, eng=split, fused=False)
            split.close()


@pytest.mark.parametrize("name", NAMES)
def test_sub_ranges(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_sub_ranges(torch_cuda, s)


@pytest.mark.parametrize("name", [c.name for c in cn.TABLE if c.inverse])
def test_inverse(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_inverse(torch_cuda, s)


@pytest.mark.parametrize("name", NAMES)
def test_identical_pairs(torch_cuda, name):
    s = case(torch_cuda, name)
    with timed(torch_cuda, name):
        check_identical_pairs(torch_cuda, s)


@pytest.mark.parametrize("name", [c.name for c in cn.TABLE if c.channels == 12])
def test_a_stream_at_8_modulo_16_bytes_gives_the_same_bytes(torch_cuda, name):
    """twelve channels from a stream 8 bytes past a 16-byte boundary: the 4096-point family then takes the narrow de-interleave for the whole
    stream (deinterleave.hip: the 16-byte kernel needs an aligned stream)"""
    torch = torch_cuda
    s = case(torch, name)
    with timed(torch, name):
        dev = to_dev(torch, s.pcm, offset_floats=2)
        assert torch.equal(words(torch, s.eng.stft_batch(dev)), words(torch, s.rows)), name
        assert torch.equal(words(torch, s.eng.stft_batch_complex(dev)), words(torch, s.cx)), name
        assert torch.equal(words(torch, s.eng.bands_batch(dev)), words(torch, s.eng.bands_batch(s.dev))), name
        assert torch.equal(words(torch, s.eng.render_batch(dev)), words(torch, s.eng.render_batch(s.dev))), name
        with mel_banks(s.eng, powers=(2,)) as fbs:
            assert torch.equal(words(torch, fbs[2].batch(dev)), words(torch, fbs[2].batch(s.dev))), name
            assert torch.equal(words(torch, fbs[2].cross_batch(dev)), words(torch, fbs[2].cross_batch(s.dev))), name


# ---- the cap rows: one test per row, so that 1 GiB streams and rows live once ---------------------------------------------------------------
@pytest.mark.parametrize("name", CAP_NAMES)
def test_cap_row(torch_cuda, name):
    """32 768 channels.  The 16384-point row (1 GiB in, 1 GiB out) is the one case allowed more than a few seconds: its wall time is in
    profiles/channel_counts.txt.  Every row is compared, on the device."""
    torch = torch_cuda
    c = cn.CASE[name]
    t0 = time.perf_counter()
    # the rows the workspace holds of a Welch call (psd, csd): none at W 2048 and W 8192 -- a frame per piece, two rows of workspace --,
    # fewer than a block of 32 and its partial at W 64 and W 735 -- a block in pieces --, and at W 23 two blocks and one
    caps = (ba.welch_cap(c.W, c.pairs, False), ba.welch_cap(c.W, c.pairs, True))
    assert caps == {"k1_h256_cap": (0, 0), "k16_h512_cap": (0, 0), "mixed_w735_runtime_cap": (2, 1), "generic_w64_cap": (24, 12),
                    "bluestein_w23_cap": (69, 34)}[name]
    assert caps == (0, 0) or caps[0] < 33 or name == "bluestein_w23_cap"
    for cross in (False, True):
        plan = ba.welch_ranges(c.W, c.pairs, cross, c.frames, ba.WELCH_MAX, True)
        assert plan.workspace_rows <= max(plan.cap, 2) and (plan.piece == 1) == (plan.cap <= 2), (name, plan)
    s = State(torch, c)
    steps = [("build", time.perf_counter() - t0)]
    todo = [("route", lambda: check_route(s)), ("truth", lambda: check_truth(torch, s)), ("derived", lambda: check_derived(torch, s)),
            ("sub-ranges", lambda: check_sub_ranges(torch, s))]
    if c.inverse:
        todo.append(("inverse", lambda: check_inverse(torch, s)))
    todo.append(("identical pairs", lambda: check_identical_pairs(torch, s)))
    for what, step in todo:
        t1 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        steps.append((what, time.perf_counter() - t1))
    _wall[name] = time.perf_counter() - t0
    print(f"CHANNEL-CAP-STEPS {name} " + ", ".join(f"{w} {t:.2f} s" for w, t in steps))
    s.eng.close()
    del s
    torch.cuda.empty_cache()


def test_cap_row_of_the_4096_point_kernel_on_the_two_kernel_route(torch_cuda):
    """SGX_FLAG_NO_FUSED_RENDER at 32 768 channels, a case of its own: every call of the 4096-point family is 16 384 launches there"""
    torch = torch_cuda
    c = cn.CASE["k1_h256_cap"]
    name = c.name + " (two-kernel)"
    with timed(torch, name):
        s = State(torch, c)
        split = engine(c, fused_render=False)
        assert split.info.render_path & 1 == 0
        check_derived(torch, s, eng=split, fused=False)
        split.close()
        s.eng.close()
    del s
    torch.cuda.empty_cache()


# ---- 7. compute-unit limits ----------------------------------------------------------------------------------------------------------------
def every_output(torch, s):
    eng, dev, F = s.eng, s.dev, s.c.frames
    with mel_banks(eng) as fbs:
        out = {"rows": eng.stft_batch(dev), "half rows": eng.stft_batch_f16(dev), "complex rows": eng.stft_batch_complex(dev),
               "pixels": eng.render_batch(dev), "bands": eng.bands_batch(dev), "fbank 2": fbs[2].batch(dev), "fbank 1": fbs[1].batch(dev),
               "cross": fbs[2].cross_batch(dev), "inverse": eng.istft_batch(s.cx)}
        for g in peak_groups(F):
            out[f"peak {g}"] = eng.bands_peak_batch(dev, g)
        return {k: words(torch, v).clone() for k, v in out.items()}


@pytest.mark.parametrize("name", cn.CU_ROWS)
def test_compute_unit_limits_around_the_pair_count(torch_cuda, name):
    torch = torch_cuda
    s = case(torch, name)
    with timed(torch, name):
        eng = s.eng
        dcu = torch.cuda.get_device_properties(0).multi_processor_count
        assert eng.cu_limit == dcu
        want = every_output(torch, s)
        assert torch.equal(want["rows"], words(torch, s.rows)) and torch.equal(want["complex rows"], words(torch, s.cx))
        try:
            for n in cn.cu_limits(s.c.pairs):
                eng.set_cu_limit(n)
                assert eng.cu_limit == n
                got = every_output(torch, s)
                for what in want:
                    assert torch.equal(got[what], want[what]), (name, "limit", n, what, "differs from the device's own count")
        finally:
            eng.set_cu_limit(0)
        assert eng.cu_limit == dcu


# ---- 8. sgx_process_one --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in cn.TABLE if c.channels == 6])
def test_process_one_is_one_lr_frame(torch_cuda, name):
    """include/sgx.h: one (l, r) frame whatever the context's channel count"""
    s = case(torch_cuda, name)
    c = s.c
    with timed(torch_cuda, name):
        lr = np.ascontiguousarray(cn.frame_of(c, s.pcm, 2)[:, 2:4])
        got = s.eng.process_one(lr)
        assert got is not None and got.shape == (c.W - 1, 2)
        err = mags_error(got, es.truth_frame(lr, c.W), c.route.floor)
        print(f"CHANNEL-PROCESS-ONE {name}: {err:.4f} (bound {c.bound})")
        assert err <= c.bound, (name, err)
        # ... and the bytes of a two-channel context's: sgx_process_one picks the family by the call's two channels on any context
        two = engine(c, channels=2)
        want = two.process_one(lr)
        two.close()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, "differs from a two-channel context's process_one")


# ---- 9. the noise generator ----------------------------------------------------------------------------------------------------------------
def test_white_noise_of_six_channels(torch_cuda):
    s = case(torch_cuda, "generic_w64_ch6")
    n, seed = 4099, 0x5EED0042
    got = s.eng.white_noise(n, seed=seed, channels=6).cpu().numpy().reshape(n, 6)
    for ch in range(6):
        assert np.array_equal(got[:, ch], oracle.white_noise(n, seed=seed + ch)), ch
    own = s.eng.white_noise(n, seed=seed).cpu().numpy().reshape(n, 6)     # (the context's own channel count)
    assert np.array_equal(own, got)


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_channel_counts(torch_cuda):
    from spectrogram_rs_amd import SgxError, SpectrogramEngine, _lib
    for channels in (0, 3, 5, 7, 32769, 32770, 65536, 2 ** 32 - 2):
        with pytest.raises(SgxError) as e:
            SpectrogramEngine(es.SR, device=0, window_samples=64, hop_samples=16, channels=channels)
        assert e.value.code == _lib.SGX_ERR_INVALID_ARG, (channels, e.value.code)
        assert "sgx_create" in str(e.value) and "channels" in str(e.value), (channels, str(e.value))
        # the process goes on: a valid create succeeds and computes
        ok = SpectrogramEngine(es.SR, device=0, window_samples=64, hop_samples=16, channels=6)
        assert ok.channels == 6 and ok.pairs == 3
        assert bool(torch_cuda.isfinite(ok.stft_batch(ok.white_noise(64 + 16))).all())
        ok.close()
    top = SpectrogramEngine(es.SR, device=0, window_samples=64, hop_samples=16, channels=cn.CAP)
    assert (top.channels, top.pairs) == (cn.CAP, cn.CAP // 2)
    top.close()


def test_wall_times(torch_cuda):
    """(last: the wall time of every case, summed over its tests, for profiles/channel_counts.txt)"""
    for name, t in _wall.items():
        print(f"CHANNEL-TIME {name} {t:.2f} s")
    slow = {n: t for n, t in _wall.items() if n != "k16_h512_cap"}
    if slow:
        worst = max(slow, key=slow.get)
        print(f"CHANNEL-TIME slowest but the 16384-point cap row: {worst} {slow[worst]:.2f} s")

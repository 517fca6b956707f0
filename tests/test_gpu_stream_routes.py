"""Every route and entry point on a stream of the caller's that is held back (tests/stream_cases.py: the table).

Every other GPU file runs on torch's default stream, the legacy NULL stream, where a helper pass launched on stream 0 is ordered exactly
like one launched on the context's stream.  Here
  1  every row of edge_signals.ROUTES runs every entry point its route serves, straight through the C ABI (no wrapper rebinds the stream),
     on a non-default stream that a sleep kernel holds back: the inputs are quiet NaN until the noise kernel, enqueued first on that stream,
     has run, the outputs are prefilled, and the context's own buffers hold another seed's state.  A kernel, copy or memset placed on
     another stream runs before its input exists.  The host must have enqueued everything before the stream wakes (nothing in the steady
     state of an entry point waits on the host), and every output is bit for bit what the same calls give on the NULL stream;
  2  so do sgx_view_write_rows / sgx_view_draw, sgx_image_write_columns / sgx_image_read, sgx_render_mags on one context per kernel body,
     sgx_magnitude_in on both of its instantiations, and a Welch call whose one column is carried and whose blocks are pieced;
  3  a context that the wrapper rebinds from a busy stream to another (SpectrogramEngine binds to torch's current stream before every
     call) has its later work ordered behind its earlier work, on the device; rebinding to the same stream costs no wait.
Nothing here has a tolerance.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import bounds_arena as ba
import edge_signals as es
import far_offsets as fo
import fbank_reference as fr
import stream_cases as sc
from test_gpu_streams import SLEEP_CYCLES

pytestmark = pytest.mark.gpu

NAN = float("nan")
PIXEL_FILL = 0xA5


class Gpu:
    def __init__(self, torch):
        self.torch = torch
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]   # with the NULL stream: three, once per module
        self.turn = 0

    def next_stream(self):
        self.turn += 1
        return self.streams[self.turn % 2]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    g = Gpu(torch)
    assert all(s.cuda_stream != 0 for s in g.streams)
    yield g
    torch.cuda.synchronize()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def same_bytes(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def buffer(torch, shape, dtype, fill):
    """a fresh device buffer: as it comes, or (the held run) quiet NaN for an input, -1 for floats and 0xA5 for pixels of an output"""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def hold(g, eng, enqueue, what):
    """steps e and f: bind the context to a non-default stream, put a sleep on it, enqueue with no host synchronisation, and say whether the
    host was ahead of the stream when it had enqueued everything; one sgx_sync"""
    torch = g.torch
    S = g.next_stream()
    torch.cuda.synchronize()
    eng._check(eng._lib.sgx_set_stream(eng._ctx, C.c_void_p(S.cuda_stream)))
    with torch.cuda.stream(S):
        torch.cuda._sleep(SLEEP_CYCLES)
    try:
        enqueue(S)
        pending = not S.query()
    finally:
        eng.sync()
    assert S.query(), (what, "sgx_sync returned before the context's stream was done")
    assert pending, (what, "the stream was idle when the host had enqueued everything: an entry point waited on the host in its steady state")
    return S


# ---- 1: every row of ROUTES ---------------------------------------------------------------------------------------------------------------
class RouteCalls:
    """the calls of one run of a row, through the C ABI only, into buffers of their own"""

    def __init__(self, torch, eng, r, entries, held, fb):
        self.torch, self.eng, self.lib, self.r, self.entries, self.fb = torch, eng, eng._lib, r, entries, fb
        F = self.F = sc.frames_of(r)
        n = self.n = (F - 1) * r.H + r.W
        Cn, P, M, R = r.channels, eng.pairs, eng.M, eng.R
        f32, u8 = torch.float32, torch.uint8
        flt, pix = (-1.0, PIXEL_FILL) if held else (None, None)
        pcm = buffer(torch, (n * Cn + 1,), f32, NAN if held else None)
        self.pcm = pcm[1:] if r.align4 else pcm[:n * Cn]
        assert self.pcm.data_ptr() % 8 == (4 if r.align4 else 0)
        cols = -(-F // sc.PEAK_GROUP)
        self.out = {
            "stft": buffer(torch, (F, P, M, 2), f32, flt), "f16": buffer(torch, (F, P, M, 2), torch.float16, flt),
            "complex": buffer(torch, (F, P, M, 2, 2), f32, flt), "render": buffer(torch, (F, P, R, 4), u8, pix),
            "bands": buffer(torch, (F, P, R, 2), f32, flt), "peak_3": buffer(torch, (cols, P, R, 2), f32, flt),
            "render_mags": buffer(torch, (F * P, R, 4), u8, pix), "magnitude_in": buffer(torch, (F * P, R, 2), f32, flt),
            "render_bands": buffer(torch, (F * P, R, 4), u8, pix), "checksum_add": torch.zeros(1, dtype=torch.int64, device="cuda"),
            "fbank": buffer(torch, (F, P, fb.n_filters, 2), f32, flt), "fbank_mags": buffer(torch, (F * P, fb.n_filters, 2), f32, flt),
            "fbank_cross_spec": buffer(torch, (F * P, fb.n_filters, 4), f32, flt),
            "psd_3": buffer(torch, (cols, P, M, 2), f32, flt), "psd_mags": buffer(torch, (cols, P, M, 2), f32, flt),
            "csd_spec": buffer(torch, (cols, P, M, 4), f32, flt),
        }
        if "csd_3" in entries:
            self.out["csd_3"] = buffer(torch, (cols, P, M, 4), f32, flt)
        if "fbank_cross" in entries:
            self.out["fbank_cross"] = buffer(torch, (F, P, fb.n_filters, 4), f32, flt)
        if "istft" in entries:
            self.out["istft"] = buffer(torch, (n, Cn), f32, flt)
        ends = eng.bin_edges()
        self.ranges = np.ascontiguousarray(np.stack([ends[:-1], ends[1:]], 1), np.float32)   # the context's own edges

    def enqueue(self, seed):
        e, lib, o, r, F, n = self.eng, self.lib, self.out, self.r, self.F, self.n
        ck, ctx, got = e._check, e._ctx, C.c_size_t(0)
        ck(lib.sgx_synth_white_noise(ctx, ptr(self.pcm), 0, n, r.channels, seed))
        for entry in self.entries:
            if entry in ("stft", "f16", "complex", "render", "bands"):
                ck(getattr(lib, sc.SYMBOL[entry])(ctx, ptr(self.pcm), n, 0, F, ptr(o[entry]), C.byref(got)))
                assert got.value == F, (r.name, entry)
            elif entry == "peak_3":
                ck(lib.sgx_bands_peak_batch(ctx, ptr(self.pcm), n, 0, F, sc.PEAK_GROUP, ptr(o[entry]), C.byref(got)))
                assert got.value == o[entry].shape[0], (r.name, entry)
            elif entry == "istft":
                ck(lib.sgx_istft_batch(ctx, ptr(o["complex"]), F, 0, n, ptr(o[entry]), C.byref(got)))
                assert got.value == n, (r.name, entry)
            elif entry == "render_mags":
                ck(lib.sgx_render_mags(ctx, ptr(o["stft"]), F * e.pairs, ptr(o[entry])))
            elif entry == "magnitude_in":
                ck(lib.sgx_magnitude_in(ctx, ptr(o["stft"]), F * e.pairs, self.ranges.ctypes.data_as(C.c_void_p), e.R, ptr(o[entry])))
            elif entry == "render_bands":
                ck(lib.sgx_render_bands(ctx, ptr(o["bands"]), F * e.pairs, ptr(o[entry])))
            elif entry in ("fbank", "fbank_cross"):
                ck(getattr(lib, sc.SYMBOL[entry])(self.fb._h, ptr(self.pcm), n, 0, F, ptr(o[entry]), C.byref(got)))
                assert got.value == F, (r.name, entry)
            elif entry in ("fbank_mags", "fbank_cross_spec"):
                ck(getattr(lib, sc.SYMBOL[entry])(self.fb._h, ptr(o[sc.READS[entry]]), F * e.pairs, ptr(o[entry])))
            elif entry in ("psd_3", "csd_3"):
                ck(getattr(lib, sc.SYMBOL[entry])(ctx, ptr(self.pcm), n, 0, F, sc.PEAK_GROUP, ptr(o[entry]), C.byref(got)))
                assert got.value == o[entry].shape[0], (r.name, entry)
            elif entry in ("psd_mags", "csd_spec"):
                ck(getattr(lib, sc.SYMBOL[entry])(ctx, ptr(o[sc.READS[entry]]), F, sc.PEAK_GROUP, ptr(o[entry]), C.byref(got)))
                assert got.value == o[entry].shape[0], (r.name, entry)
            else:
                assert entry == "checksum_add"
                ck(lib.sgx_checksum_add(ctx, ptr(o["stft"]), o["stft"].numel() * 4, 0, ptr(o[entry])))


def open_route(r, **extra):
    """a context of a row, its kernel, render_path bits and fused routes asserted first (as tests/test_gpu_edges.py::test_route does)"""
    from spectrogram_rs_amd import SpectrogramEngine
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", **r.engine_kwargs(), **extra)
    try:
        info = eng.info
        assert info.stft_kernel == r.kernel, (r.name, info.stft_kernel)
        assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (r.name, info.render_path)
        if r.bands_fused is not None:
            assert eng.bands_fused == r.bands_fused, (r.name, eng.bands_fused)
        assert eng.bands_peak_fused == sc.peak_fused(r), (r.name, eng.bands_peak_fused)
        assert eng.istft_supported() == int(sc.istft_served(r)), r.name
        assert eng.psd_fused == eng.csd_fused == sc.psd_fused(r) == 0, r.name
    except BaseException:
        eng.close()
        raise
    return eng


@pytest.mark.parametrize("row", list(sc.by_row()))
def test_route_on_a_held_stream(gpu, row):
    torch = gpu.torch
    r, entries = es.ROUTE[row], sc.by_row()[row]
    eng = open_route(r)
    try:
        # the bank of the sweep, made before any sleep kernel is queued (sgx_fbank_create may wait for its own uploads)
        fb = eng.filterbank(*fr.edge_bank(eng.M), power=2)
        assert (fb.fused, fb.cross_fused) == (ba.fbank_fused(r), ba.fbank_fused(r, cross=True)), (row, fb.fused, fb.cross_fused)
        assert eng._lib.sgx_set_stream(eng._ctx, None) == 0                 # the NULL stream
        warm, want = RouteCalls(torch, eng, r, entries, False, fb), RouteCalls(torch, eng, r, entries, False, fb)
        warm.enqueue(sc.SEED_A)          # a: the lazy allocations, the inverse's tables, the range tables
        want.enqueue(sc.SEED_B)          # b: the reference
        warm.enqueue(sc.SEED_A)          # c: the context's own buffers hold another stream's state
        held = RouteCalls(torch, eng, r, entries, True, fb)                 # d
        hold(gpu, eng, lambda S: held.enqueue(sc.SEED_B), row)              # e, f
        assert not same_bytes(torch, warm.out["stft"], want.out["stft"])    # (the stale state IS another state)
        render_fused, bands_fused = bool(eng.info.render_path & 1), bool(eng.bands_fused)
        wrong = [e for e in entries if not same_bytes(torch, held.out[e], want.out[e])]
        for e in entries:
            tags = ",".join(sorted(sc.helpers(r, e, render_fused, bands_fused))) or "-"
            state = "same" if e not in wrong else "DOWNSTREAM" if sc.READS.get(e) in wrong else "DIFFERS"
            print(f"STREAM-CASE {row} {e} {state} helpers={tags}")
        assert not wrong, (row, "differ from the same calls on the NULL stream",
                           [e for e in wrong if sc.READS.get(e) not in wrong], "and, reading those,", [e for e in wrong if sc.READS.get(e) in wrong])
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- 2: the stand-alone objects --------------------------------------------------------------------------------------------------------------
def small_engine(case, **extra):
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(es.SR, device=0, gradient="viridis", window_samples=case.W, hop_samples=case.H, channels=case.channels, **extra)


@pytest.mark.parametrize("case", sc.VIEW_CASES, ids=lambda c: c.name)
def test_view_on_a_held_stream(gpu, case):
    """noise -> half rows -> sgx_view_write_rows (a copy per piece of the ring) -> sgx_view_draw.  One view: its first draw uploads the
    palette synchronously, the warm-up takes that; every second write ends at the offset the ring began with"""
    torch = gpu.torch
    eng = small_engine(case)
    view = eng.view(case.viewport)
    lib, ctx, F = eng._lib, eng._ctx, case.frames
    n = (F - 1) * case.H + case.W
    assert eng.pairs == 1

    class Run:
        def __init__(self, held):
            self.pcm = buffer(torch, (n * case.channels,), torch.float32, NAN if held else None)
            self.rows = buffer(torch, (F, eng.M, 2), torch.float16, -1.0 if held else None)
            self.picture = buffer(torch, (case.height, case.width, 4), torch.float32, -1.0 if held else None)
            self.offset = None

        def enqueue(self, seed):
            got, off = C.c_size_t(0), C.c_uint32(0)
            eng._check(lib.sgx_synth_white_noise(ctx, ptr(self.pcm), 0, n, case.channels, seed))
            eng._check(lib.sgx_stft_batch_f16(ctx, ptr(self.pcm), n, 0, F, ptr(self.rows), C.byref(got)))
            eng._check(lib.sgx_view_write_rows(view._h, ptr(self.rows), F, C.byref(off)))
            eng._check(lib.sgx_view_draw(view._h, case.width, case.height, ptr(self.picture)))
            self.offset = off.value

    try:
        warm, want, held = Run(False), Run(False), Run(True)
        warm.enqueue(sc.SEED_A)
        want.enqueue(sc.SEED_B)
        warm.enqueue(sc.SEED_A)
        hold(gpu, eng, lambda S: held.enqueue(sc.SEED_B), case.name)
        assert held.offset == want.offset == 0 and warm.offset == F % case.viewport
        assert not same_bytes(torch, warm.picture, want.picture)
        assert same_bytes(torch, held.rows, want.rows), (case.name, "the half rows differ")
        assert same_bytes(torch, held.picture, want.picture), (case.name, "the drawn viewport differs from the NULL stream's")
    finally:
        torch.cuda.synchronize()
        view.close()
        eng.close()


@pytest.mark.parametrize("case", sc.IMAGE_CASES, ids=lambda c: c.name)
def test_image_on_a_held_stream(gpu, case):
    """noise -> pixel columns -> sgx_image_write_columns (more columns than the image is wide) -> sgx_image_read as it lies (a copy) and
    scrolled (a kernel: the offset is not 0).  One fresh image per run: a new image owes nothing to a first call"""
    torch = gpu.torch
    eng = small_engine(case)
    lib, ctx, F = eng._lib, eng._ctx, sc.FRAMES
    n = (F - 1) * case.H + case.W
    assert eng.pairs == 1 and eng.W != 2048

    class Run:
        def __init__(self, held):
            self.img = eng.image(case.width)
            self.pcm = buffer(torch, (n * case.channels,), torch.float32, NAN if held else None)
            self.rgba = buffer(torch, (F, eng.R, 4), torch.uint8, PIXEL_FILL if held else None)
            self.flat = buffer(torch, (eng.R, case.width, 4), torch.uint8, PIXEL_FILL if held else None)
            self.scrolled = buffer(torch, (eng.R, case.width, 4), torch.uint8, PIXEL_FILL if held else None)
            self.offset = None

        def enqueue(self, seed):
            got, off = C.c_size_t(0), C.c_uint32(0)
            eng._check(lib.sgx_synth_white_noise(ctx, ptr(self.pcm), 0, n, case.channels, seed))
            eng._check(lib.sgx_render_batch(ctx, ptr(self.pcm), n, 0, F, ptr(self.rgba), C.byref(got)))
            eng._check(lib.sgx_image_write_columns(self.img._h, ptr(self.rgba), F, C.byref(off)))
            eng._check(lib.sgx_image_read(self.img._h, 0, ptr(self.flat)))
            eng._check(lib.sgx_image_read(self.img._h, 1, ptr(self.scrolled)))
            self.offset = off.value

    runs = []
    try:
        warm, want, held = Run(False), Run(False), Run(True)
        runs = [warm, want, held]
        warm.enqueue(sc.SEED_A)
        want.enqueue(sc.SEED_B)
        hold(gpu, eng, lambda S: held.enqueue(sc.SEED_B), case.name)
        assert held.offset == want.offset == F % case.width != 0
        assert not same_bytes(torch, warm.scrolled, want.scrolled) and not same_bytes(torch, want.flat, want.scrolled)
        for name in ("rgba", "flat", "scrolled"):
            assert same_bytes(torch, getattr(held, name), getattr(want, name)), (case.name, name, "differs from the NULL stream's")
    finally:
        torch.cuda.synchronize()
        for run in runs:
            run.img.close()
        eng.close()


@pytest.mark.parametrize("case", sc.WELCH_CASES, ids=lambda c: c.name)
def test_welch_carried_and_pieced_on_a_held_stream(gpu, case):
    """One column whose float64 sums wait in the context's carry row between ranges, every block's rows taken a few frames at a time (the
    later pieces resume the block's partial): several rows launches with kernel 11's passes, block launches and a combine per range, all
    behind the sleep.  The workspace is warmed by a call that carries nothing, so the carry row is grown on the held stream by the call
    under test; the reference runs on the NULL stream afterwards, on a fresh context."""
    from spectrogram_rs_amd import SpectrogramEngine
    torch = gpu.torch
    plan = ba.welch_ranges(case.W, case.channels // 2, case.cross, case.frames, case.group, True)
    assert plan.carried and plan.piece and plan.resumed and len(plan.ranges) >= 2
    short = ba.welch_ranges(case.W, case.channels // 2, case.cross, case.frames, 1, True)
    assert not short.carried and short.workspace_rows >= plan.workspace_rows      # the warm-up grows the whole workspace, and no carry row
    kw = dict(window_samples=case.W, hop_samples=case.H, channels=case.channels, large_transforms=True)
    n = (case.frames - 1) * case.H + case.W
    fn = "sgx_csd_batch" if case.cross else "sgx_psd_batch"

    def run(eng, pcm, out, seed, group):
        got = C.c_size_t(0)
        eng._check(eng._lib.sgx_synth_white_noise(eng._ctx, ptr(pcm), 0, n, case.channels, seed))
        eng._check(getattr(eng._lib, fn)(eng._ctx, ptr(pcm), n, 0, case.frames, group, ptr(out), C.byref(got)))
        return got.value

    engines = []
    try:
        eng = SpectrogramEngine(es.SR, device=0, **kw)
        engines.append(eng)
        assert eng.info.stft_kernel == 11 and eng.info.mags_bytes_per_frame == ba.mags_bytes_per_frame(case.W, eng.pairs)
        comps = 4 if case.cross else 2
        assert eng._lib.sgx_set_stream(eng._ctx, None) == 0
        pcm = buffer(torch, (n * case.channels,), torch.float32, None)
        scratch = buffer(torch, (case.frames, eng.pairs, eng.M, comps), torch.float32, None)
        assert run(eng, pcm, scratch, sc.SEED_A, 1) == case.frames                 # the workspace and kernel 11's scratch: another seed's state
        del scratch
        torch.cuda.synchronize()
        pcm.fill_(NAN)
        held = buffer(torch, (1, eng.pairs, eng.M, comps), torch.float32, -1.0)
        cols = []
        hold(gpu, eng, lambda S: cols.append(run(eng, pcm, held, sc.SEED_B, case.group)), case.name)
        assert cols == [1]
        ref = SpectrogramEngine(es.SR, device=0, **kw)
        engines.append(ref)
        want = buffer(torch, (1, eng.pairs, eng.M, comps), torch.float32, None)
        pcm2 = buffer(torch, (n * case.channels,), torch.float32, None)
        assert run(ref, pcm2, want, sc.SEED_B, case.group) == 1
        torch.cuda.synchronize()
        assert same_bytes(torch, pcm, pcm2) and bool(torch.isfinite(want).all())
        assert same_bytes(torch, held, want), (case.name, "differs from the NULL stream's")
    finally:
        torch.cuda.synchronize()
        for e in engines:
            e.close()


def lds_cap(torch):
    """the launchers' min(the device's opt-in LDS, 160 KiB)"""
    hip = C.CDLL("libamdhip64.so")
    optin = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(optin), 75, 0) == 0 and optin.value >= torch.cuda.get_device_properties(0).shared_memory_per_block
    return min(optin.value, 160 << 10)


def pixel_ranges(n):
    edges = np.geomspace(32.0, 20000.0, n + 1)
    return np.ascontiguousarray(np.stack([edges[:-1], edges[1:]], 1), np.float32)


@pytest.mark.parametrize("case", sc.PIXEL_CASES, ids=lambda c: c.name)
def test_pixel_stage_on_a_held_stream(gpu, case):
    """sgx_render_mags on one context per kernel body, sgx_magnitude_in on both of its instantiations: the magnitudes (squares of the
    context's noise) are made on the held stream too"""
    from pixel_plans import ramp
    from spectrogram_rs_amd import SpectrogramEngine
    torch = gpu.torch
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", window_samples=case.W, hop_samples=max(case.W // 2, 1), channels=2, rows=case.R,
                            large_transforms=case.large)
    try:
        if case.n_lut != 256:
            eng.set_gradient(ramp(case.n_lut))
        body = fo.pixel_body(case.entry, eng.M, eng.info.total_samples_per_column, case.n_lut, lds_cap(torch))
        assert body == case.body, (case.name, body)
        lib, ctx, cols, iw = eng._lib, eng._ctx, case.cols, eng.M * 2
        ranges = pixel_ranges(case.n_ranges)

        class Run:
            def __init__(self, held):
                self.src = buffer(torch, (cols * iw,), torch.float32, NAN if held else None)
                if case.entry == "render_mags":
                    self.out = buffer(torch, (cols, eng.R, 4), torch.uint8, PIXEL_FILL if held else None)
                else:
                    self.out = buffer(torch, (cols, case.n_ranges, 2), torch.float32, -1.0 if held else None)

            def enqueue(self, seed, S=None):
                eng._check(lib.sgx_synth_white_noise(ctx, ptr(self.src), 0, cols * iw, 1, seed))
                with torch.cuda.stream(S if S is not None else torch.cuda.default_stream()):
                    self.src.mul_(self.src).add_(1e-7)          # magnitudes from 1e-7 to 1, on the stream the noise is on
                if case.entry == "render_mags":
                    eng._check(lib.sgx_render_mags(ctx, ptr(self.src), cols, ptr(self.out)))
                else:
                    eng._check(lib.sgx_magnitude_in(ctx, ptr(self.src), cols, ranges.ctypes.data_as(C.c_void_p), case.n_ranges, ptr(self.out)))

        warm, want, held = Run(False), Run(False), Run(True)
        warm.enqueue(sc.SEED_A)
        want.enqueue(sc.SEED_B)
        hold(gpu, eng, lambda S: held.enqueue(sc.SEED_B, S), case.name)
        assert not same_bytes(torch, warm.out, want.out)
        assert same_bytes(torch, held.src, want.src) and bool(torch.isfinite(want.src).all())
        assert same_bytes(torch, held.out, want.out), (case.name, case.body, "differs from the NULL stream's")
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- 3: rebinding a busy context (through the wrapper: it is the wrapper that rebinds) -------------------------------------------------------
REBIND_FRAMES = 40


def rebind_engine(kw):
    from spectrogram_rs_amd import SpectrogramEngine
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", **kw)
    # the 16384-point kernel, pixels and bands in two kernels through the workspace (a mono stream: through the duplicated plane first)
    assert eng.info.stft_kernel == 10 and eng.info.render_path & 1 == 0 and eng.bands_fused == 0, kw
    return eng


def rebind_setup(torch, eng, method, first_stream):
    """two streams of samples, their results from two calls made one after the other on the NULL stream, the context's buffers left in the
    state of the first, and two prefilled outputs (out=: the caching allocator plays no part).  A method "fbank_<m>" is FilterBank.<m> of
    a bank created while the context is bound to first_stream."""
    n = (REBIND_FRAMES - 1) * eng.H + eng.W
    if method.startswith("fbank_"):
        with torch.cuda.stream(first_stream):
            fb = eng.filterbank(*fr.edge_bank(eng.M), power=2)     # (the wrapper binds the context to first_stream, then creates)
        assert fb.fused == 0
        f = getattr(fb, method[len("fbank_"):])
    else:
        f = getattr(eng, method)
    pcm = [eng.white_noise(n, seed=s) for s in (sc.SEED_A, sc.SEED_B)]
    want = [f(p).clone() for p in pcm]
    f(pcm[0])
    assert not same_bytes(torch, want[0], want[1])
    fill = PIXEL_FILL if want[0].dtype == torch.uint8 else -1.0
    outs = [torch.full_like(w, fill) for w in want]
    torch.cuda.synchronize()
    return f, pcm, want, outs


@pytest.mark.parametrize("name,kw,method", sc.REBIND_CASES, ids=[c[0] for c in sc.REBIND_CASES])
def test_rebinding_a_busy_context_orders_the_new_stream_behind_the_old(gpu, name, kw, method):
    torch = gpu.torch
    a, b = gpu.streams
    eng = rebind_engine(kw)
    try:
        f, pcm, want, outs = rebind_setup(torch, eng, method, a)
        with torch.cuda.stream(a):
            torch.cuda._sleep(SLEEP_CYCLES)
            f(pcm[0], out=outs[0])
        with torch.cuda.stream(b):
            f(pcm[1], out=outs[1])
        ahead = not a.query()                 # the rebinding did not wait on the host
        b.synchronize()                       # b only
        ordered = a.query()
        torch.cuda.synchronize()
        print(f"STREAM-REBIND {name}: host ahead of stream a after both calls: {ahead}; a done when b is: {ordered}; "
              f"bytes of call 1 / call 2 right: {same_bytes(torch, outs[0], want[0])} / {same_bytes(torch, outs[1], want[1])}")
        assert ahead, (name, "a rebinding waited on the host")
        assert ordered, (name, "stream b finished the context's second call while its first was still pending on stream a: the two share the "
                               "workspace, and nothing ordered them")
        assert same_bytes(torch, outs[0], want[0]) and same_bytes(torch, outs[1], want[1]), (name, "differs from the two calls made serially")
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_rebinding_to_the_same_stream_keeps_the_host_ahead(gpu):
    torch = gpu.torch
    a = gpu.streams[0]
    name, kw, method = sc.REBIND_CASES[0]
    eng = rebind_engine(kw)
    try:
        f, pcm, want, outs = rebind_setup(torch, eng, method, a)
        with torch.cuda.stream(a):
            torch.cuda._sleep(SLEEP_CYCLES)
            f(pcm[0], out=outs[0])            # the wrapper binds to a ...
            f(pcm[1], out=outs[1])            # ... and again to a: nothing to order, nothing to wait for
            pending = not a.query()
        a.synchronize()
        assert pending, "the host did not run ahead of the held stream: binding to the stream the context is on waited"
        assert same_bytes(torch, outs[0], want[0]) and same_bytes(torch, outs[1], want[1])
    finally:
        torch.cuda.synchronize()
        eng.close()

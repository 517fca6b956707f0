"""Every route and batch entry point across the 2 GiB and 4 GiB marks (tests/far_offsets.py: the marks, the arenas and the case tables), all
through SpectrogramEngine and the C ABI.

An offset truncated to 32 bits wraps to a lower, valid address of the same buffer: nothing faults, the call returns wrong rows.  Here
  1  every row of edge_signals.ROUTES reads five frames around byte 2^31, byte 2^32, float 2^31 and float 2^32 of its stream, twice
     (first_frame even and odd; n_samples the last frame's end and the whole arena), on every batch entry point;
  2  every kernel family runs with a hop of just below and just above 2^31 and 2^32 bytes;
  3  every kernel family runs at H = 1 around frame 2^31 and frame 2^32, and the inverse (one context per route) resynthesises frames
     whose t H and first_sample lie beyond 2^32;
  4  every kernel family writes magnitudes, half rows, complex rows, pixel columns, bands and peak columns past 2^31 and 2^32 bytes; so
     do sgx_istft_batch (hops beyond the window: the gaps exact zeros) and, with their input past 2^32 bytes as well, sgx_render_mags,
     sgx_magnitude_in and sgx_render_bands, one context per kernel body, the body derived on the device from the launchers' own
     quantities.  The filterbank calls write 1024 single-bin sums per frame past both marks on the fused family and on one workspace
     family, and their stages alone (sgx_fbank_mags, sgx_fbank_cross_spec) on 64-point columns; their probe rows are held to the header's
     definition (tests/fbank_reference.py) bit for bit.  The Welch calls at group 1 write a column per frame past both marks on the two
     4096-point families (43 ranges of the workspace each), and their stages alone (sgx_psd_mags, sgx_csd_spec) read and write rows of 63
     bins past them at groups 1 and 2; probe rows against the header's sum order (tests/psd_reference.py), the whole by checksum against
     a torch expression over the same rows.  (Not here: sgx_image_* and sgx_view_* on rings of more than 2^32 bytes.)
The streams of 1 - 3 lie in NaN arenas where only the samples the call's frames own hold noise.  Results are compared bit for bit with
a compact replay (the same samples at the same address modulo 16 and the same frame parity in a small fresh tensor); magnitudes and
complex rows are also held to the float64 truth at the bound the project holds white noise to (conftest.KERNEL_BOUND / chirpz_bound,
test_gpu_large.LARGE_BOUND) and the row's floor.  The outputs of 4 lie in front of a guard and are prefilled: the guard must be intact,
no prefill may be left, probe rows are bit for bit what a one-frame call gives (and held to the truth or to the oracle's pixel stage),
and the checksum of the whole equals that of the same frames computed in pieces below 2^31 bytes.
Arena B (16.1 GiB) is skipped only where the device has less than the arena plus 8 GiB free.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import bounds_arena as ba
import edge_signals as es
import far_offsets as fo
import fbank_reference as fr
import oracle
import psd_reference as pr
from conftest import KERNEL_BOUND, chirpz_bound, mags_error
from test_gpu_bounds import words
from test_gpu_complex import complex_error, truth_complex
from test_gpu_large import LARGE_BOUND
from test_gpu_peak import amax_groups, same

pytestmark = pytest.mark.gpu

KINDS = ["stft", "f16", "complex", "render", "bands", "peak_3"]
NAN_I32 = ba.as_i32(ba.NAN_WORD)
SLICE_WORDS = 1 << 28   # 1 GiB: the most one device-side comparison looks at
_worst = {}


class Gpu:
    def __init__(self, torch):
        self.torch = torch
        self.arenas, self.engines = {}, {}

    def arena(self, name):
        """one allocation per module, every word the quiet NaN (int32 words)"""
        torch = self.torch
        if name not in self.arenas:
            need = fo.arena_bytes(name)
            free, _ = torch.cuda.mem_get_info()
            if name == "B" and free < need + fo.ARENA_B_HEADROOM:
                pytest.skip(f"arena B: {free} bytes free on the device, {need} + {fo.ARENA_B_HEADROOM} needed")
            self.arenas[name] = torch.full((fo.ARENA_FLOATS[name],), NAN_I32, dtype=torch.int32, device="cuda")
            print(f"FAR-ARENA {name}: {need} bytes, {free} free before it")
        return self.arenas[name]

    def open(self, r, **extra):
        """a context of a route, its kernel and render_path bits asserted first (as tests/test_gpu_edges.py::test_route does); the caller
        closes it"""
        from spectrogram_rs_amd import SpectrogramEngine
        key = (r.name, r.H, tuple(sorted(extra.items())))
        eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", **r.engine_kwargs(), **extra)
        try:
            info = eng.info
            assert info.stft_kernel == r.kernel, (key, info.stft_kernel)
            assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (key, info.render_path)
            if r.bands_fused is not None and not extra:
                assert eng.bands_fused == r.bands_fused, (key, eng.bands_fused)
        except BaseException:
            eng.close()
            raise
        return eng

    def engine(self, r, **extra):
        """the same, kept until the module ends: the rows of ROUTES as they stand, which many cases share.  (The contexts of one case --
        a large hop, H = 1 -- are opened and closed by that case: an unpaired mono W 8192 context keeps an (s, s) plane of its last call,
        17 GB at H = 2^30.)"""
        key = (r.name, r.H, tuple(sorted(extra.items())))
        if key not in self.engines:
            self.engines[key] = self.open(r, **extra)
        return self.engines[key]

    def close(self):
        self.torch.cuda.synchronize()
        for e in self.engines.values():
            e.close()
        self.engines.clear()
        self.arenas.clear()
        self.torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    g = Gpu(torch)
    yield g
    g.close()
    for k in sorted(_worst):
        print(f"FAR-WORST {k} {_worst[k]:.4f}")


def far_bank_of(eng):
    """the context's bank of the far-offset cases (far_offsets.far_bank at power 2), made once"""
    if getattr(eng, "_far_bank", None) is None:
        eng._far_bank = eng.filterbank(*fo.far_bank(eng.M), power=2)
        assert eng._far_bank.n_filters == fo.BANK_FILTERS
    return eng._far_bank


def run(eng, kind, pcm, first, n, out=None):
    if kind == "fbank":
        return far_bank_of(eng).batch(pcm, first, n, out=out)
    if kind == "fbank_cross":
        return far_bank_of(eng).cross_batch(pcm, first, n, out=out)
    if kind.startswith("peak_"):
        return eng.bands_peak_batch(pcm, int(kind[5:]), first, n, out=out)
    if kind in fo.WELCH_KINDS:
        return (eng.psd_batch if kind == "psd_1" else eng.csd_batch)(pcm, 1, first, n, out=out)
    f = {"stft": eng.stft_batch, "f16": eng.stft_batch_f16, "complex": eng.stft_batch_complex, "render": eng.render_batch,
         "bands": eng.bands_batch}[kind]
    return f(pcm, first, n, out=out)


def bound_of(r):
    if r.kernel == 11:
        return LARGE_BOUND["default"]
    return chirpz_bound(r.W) if r.kernel == 4 else KERNEL_BOUND["default"]


def cpu_noise(r, lo, hi):
    """[hi - lo][channels]: what SpectrogramEngine.white_noise(first=lo) writes (channel c: seed + c)"""
    return np.stack([oracle.white_noise(hi - lo, first=lo, seed=fo.NOISE_SEED + c) for c in range(r.channels)], 1)


class Truth:
    """the float64 truth of the frames of one case, by absolute frame index; window(t) -> [W][channels] or None"""

    def __init__(self, r, window):
        self.r, self.window, self.cache = r, window, {}

    def of(self, t):
        if t not in self.cache:
            x = self.window(t)
            self.cache[t] = None if x is None else [
                (es.truth_frame(es.frame_lr(x, p), self.r.W), truth_complex(es.frame_lr(x, p), self.r.W)) for p in range(self.r.pairs)]
        return self.cache[t]

    def hold(self, what, t, mags, cx):
        """frame t's magnitudes [pairs][M][2] and complex rows against the truth: the worst ratio to the bound"""
        r = self.r
        ref, worst = self.of(t), 0.0
        partner = self.of(t ^ 1) if r.paired else None   # (None: the stream does not hold the partner frame)
        for p in range(r.pairs):
            m_ref, c_ref = ref[p]
            m_peak = c_peak = 0.0
            if partner is not None:
                m_peak, c_peak = float(np.abs(partner[p][0]).max()), float(np.abs(partner[p][1]).max())
            if mags is not None:
                e = es.pair_error(mags[p], m_ref, r.floor, m_peak) if r.paired else mags_error(mags[p], m_ref, r.floor)
                worst = max(worst, e)
            if cx is not None:
                e = complex_error(cx[p], c_ref, r.floor, max(float(np.abs(c_ref).max()), c_peak))
                worst = max(worst, e)
        return worst / bound_of(r)


def note(family, ratio):
    _worst[family] = max(_worst.get(family, 0.0), ratio)


def compact(g, src_i, src_addr, lo, hi, rp_lo, n_floats):
    """a fresh NaN tensor of n_floats whose float rp_lo + i holds src_i[lo + i], at src_addr modulo 16 (far_offsets.replay_pad)"""
    torch = g.torch
    small = torch.full((n_floats + 4,), NAN_I32, dtype=torch.int32, device="cuda")
    pad = fo.replay_pad(src_addr, small.data_ptr())
    rep = small[pad:pad + n_floats]
    assert rep.data_ptr() % 16 == src_addr % 16
    rep[rp_lo:rp_lo + hi - lo] = src_i[lo:hi]
    return rep.view(torch.float32)


# ---- parts 1 and 3: the marks inside the stream -----------------------------------------------------------------------------------------
def check_input_case(g, case):
    torch = g.torch
    r = case.route
    C, W, H = r.channels, r.W, r.H
    eng = g.engine(r) if case.part == 1 else g.open(r)
    try:
        run_input_case(g, case, eng)
    finally:
        torch.cuda.synchronize()
        if case.part != 1:
            eng.close()


def run_input_case(g, case, eng):
    torch = g.torch
    r = case.route
    C, W, H = r.channels, r.W, r.H
    stream_i = g.arena(case.arena)[fo.base_offset(r):]
    stream = stream_i.view(torch.float32)
    if r.align4:
        assert stream.data_ptr() % 8 == 4
    truths = {}
    for first, n, n_samples in case.calls():
        lo, hi = fo.owned(r, first, n, n_samples)
        what = f"{case.id} first {first} n_samples {n_samples}"
        eng.white_noise(hi - lo, first=lo, seed=fo.NOISE_SEED, out=stream[lo * C:hi * C])
        try:
            pcm = stream[:n_samples * C]
            assert eng.num_frames(n_samples) >= first + n
            rp = fo.replay_of(r, first, lo, hi)
            rep = compact(g, stream_i, stream.data_ptr() + rp.shift * C * 4, lo * C, hi * C, rp.lo * C, rp.n_samples * C)
            res = {}
            for kind in KINDS:
                got = run(eng, kind, pcm, first, n)
                want = run(eng, kind, rep, rp.first, n)
                assert got.shape == want.shape and got.shape[0] == (-(-n // 3) if kind == "peak_3" else n), (what, kind)
                assert torch.equal(words(torch, got), words(torch, want)), (what, kind, "differs from the compact replay")
                res[kind] = got
            host = cpu_noise(r, lo, hi)

            def window(t, lo=lo, hi=hi, host=host):
                return host[t * H - lo:t * H - lo + W] if lo <= t * H and t * H + W <= hi else None
            # (the truth of a frame is the same in both calls; a partner frame only one of them owns is looked up again)
            truth = Truth(r, window)
            truth.cache = {t: v for t, v in truths.items() if v is not None}
            mags, cx = res["stft"].cpu().numpy(), res["complex"].cpu().numpy()
            ratio = max(truth.hold(what, first + j, mags[j], cx[j]) for j in range(n))
            truths.update(truth.cache)
            print(f"FAR-RATIO {what}: {ratio:.4f} of the bound {bound_of(r)}")
            note(f"part {case.part} {case.row}", ratio)
            assert ratio <= 1.0, (what, ratio, "misses the float64 truth")
        finally:
            stream_i[lo * C:hi * C] = NAN_I32
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", fo.input_cases(), ids=lambda c: c.id)
def test_stream_marks(gpu, case):
    check_input_case(gpu, case)


@pytest.mark.parametrize("case", fo.index_cases(), ids=lambda c: c.id)
def test_frame_index_marks(gpu, case):
    check_input_case(gpu, case)


# ---- part 2: the hop as the large number -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fo.hop_cases(), ids=lambda c: c.id)
def test_hop_marks(gpu, case):
    from spectrogram_rs_amd import builtin_gradient
    g, torch = gpu, gpu.torch
    r, small = case.route, case.small
    eng_small = g.engine(small)
    stream_i = g.arena(case.arena)
    stream = stream_i.view(torch.float32)
    eng = g.open(r)   # this case's own: closed below with whatever its calls made it keep
    rows_eng = None
    try:
        if r.paired:
            rows_eng = pixel_rows_engine(g, r, eng)
        run_hop_case(g, case, eng, eng_small, rows_eng, stream_i, stream, builtin_gradient("viridis"))
    finally:
        torch.cuda.synchronize()
        eng.close()
        if rows_eng is not None and rows_eng is not eng:
            rows_eng.close()


def oracle_bands(eng, mags):
    """[R][2]: the oracle's band means of one column of magnitudes [M][2] over the context's own rows"""
    sr, ends = eng.info.sample_rate_u32, eng.bin_edges()
    return np.stack([oracle.magnitude_in(mags, sr, float(ends[py]), float(ends[py + 1])) for py in range(eng.R)])


def run_hop_case(g, case, eng, eng_small, rows_eng, stream_i, stream, grad):
    torch = g.torch
    r = case.route
    C, W, H = r.channels, r.W, r.H
    for first, n, n_samples in case.calls():
        wins = fo.owned_windows(r, first, n, n_samples)
        what = f"{case.id} first {first} n_samples {n_samples}"
        for a, b in wins:
            eng.white_noise(b - a, first=a, seed=fo.NOISE_SEED, out=stream[a * C:b * C])
        try:
            pcm = stream[:n_samples * C]
            assert eng.num_frames(n_samples) >= first + n
            res = {kind: run(eng, kind, pcm, first, n) for kind in KINDS}
            if not r.paired:   # (two frames of one transform round differently from one frame alone: only the truth applies there)
                for j in range(n):
                    a = (first + j) * H
                    rep = compact(g, stream_i, stream.data_ptr() + a * C * 4, a * C, (a + W) * C, 0, W * C)
                    for kind in KINDS[:5]:
                        want = run(eng_small, kind, rep, 0, 1)
                        assert torch.equal(words(torch, res[kind][j]), words(torch, want[0])), (what, kind, j, "differs from the replay")
            host = {a: cpu_noise(r, a, b) for a, b in wins}
            truth = Truth(r, lambda t: host.get(t * H))
            mags, cx = res["stft"].cpu().numpy(), res["complex"].cpu().numpy()
            ratio = max(truth.hold(what, first + j, mags[j], cx[j]) for j in range(n))
            print(f"FAR-RATIO {what}: {ratio:.4f} of the bound {bound_of(r)}")
            note(f"part 2 {case.family}", ratio)
            assert ratio <= 1.0, (what, ratio, "misses the float64 truth")
            assert same(res["peak_3"], amax_groups(res["bands"], 3)), (what, "peak_3")
            if r.paired:   # no replay: the half rows follow the call's own rows, the pixels and the bands the oracle's pixel stage on them
                assert torch.equal(res["f16"], res["stft"].half()), (what, "f16")
                px_rows = mags if rows_eng is eng else rows_eng.stft_batch(pcm, first, n).cpu().numpy()
                px, bands = res["render"].cpu().numpy(), res["bands"].cpu().numpy()
                for j in range(n):
                    want = oracle.render_columns(px_rows[j, 0][None], eng.info.sample_rate_u32, grad, R=eng.R)[0]
                    assert np.array_equal(px[j, 0], want), (what, j, "the pixels differ from the oracle's of the engine's rows")
                    want = oracle_bands(eng, mags[j, 0])
                    assert np.array_equal(bands[j, 0].view(np.uint32), want.view(np.uint32)) or np.array_equal(bands[j, 0], want), \
                        (what, j, "the bands differ from the oracle's band means of the engine's rows")
        finally:
            for a, b in wins:
                stream_i[a * C:b * C] = NAN_I32
    torch.cuda.synchronize()


# ---- part 4: outputs past 2^31 and 2^32 bytes --------------------------------------------------------------------------------------------
ELEM = {"stft": "f32", "f16": "f16", "complex": "f32", "render": "u8", "bands": "f32", "peak_2": "f32", "fbank": "f32", "fbank_cross": "f32",
        "psd_1": "f32", "csd_1": "f32"}


def welch_terms(torch, entry, rows):
    """the summands of the Welch calls as a torch expression in float32, one kernel per product, sum and difference (nothing is
    contracted): psd rows [..., 2] of magnitudes -> m * m; csd rows [..., 4] of (a, b, c, d) -> [..., 4].  The probe rows of every case
    hold the same bits to tests/psd_reference.py's psd_terms / csd_terms."""
    if entry in ("psd_mags", "psd_1"):
        return rows * rows
    a, b, c, d = rows.unbind(-1)
    return torch.stack([a * a + b * b, c * c + d * d, a * c + b * d, b * c - a * d], -1)


def welch_means_of_two(torch, x):
    """group 2 as a torch expression: x [2 j or 2 j + 1 frames][...] -> the means of columns of two frames.  The block's chain from +0 is
    exact for its first add, so a column is (float)((double)(x0 + x1) / 2); an odd last frame is a column of its own, x / 1"""
    pairs = x[:x.shape[0] // 2 * 2].view(x.shape[0] // 2, 2, *x.shape[1:])
    out = ((pairs[:, 0] + pairs[:, 1]).double() / 2.0).float()
    return out if x.shape[0] % 2 == 0 else torch.cat([out, x[-1:] + 0.0])


def count_equal(torch, t, word):
    """how many int32 words of t equal `word`, counted on the device in slices of at most 1 GiB"""
    total = 0
    for a in range(0, t.numel(), SLICE_WORDS):
        total += int((t[a:a + SLICE_WORDS] == word).sum())
    return total


def fused_pixels_are_mixed(r, eng):
    """The 4800-point kernel writes rows only: the fused pixels of its contexts are the composite-radix kernel's, as in
    tests/test_gpu_edges.py::test_half_rows_pixels_and_bands."""
    return bool(eng.info.render_path & 1 and r.kernel == 9 and r.channels <= 2 and not eng.info.render_path & 8)


def pixel_rows_engine(g, r, eng):
    """the context whose magnitudes the fused pixels of `eng` are made of: eng itself, or one under SGX_FLAG_MIXED_GENERIC that the caller
    closes"""
    if not fused_pixels_are_mixed(r, eng):
        return eng
    from spectrogram_rs_amd import SpectrogramEngine
    return SpectrogramEngine(es.SR, device=0, mixed_generic=True, **r.engine_kwargs())


def own_rows(g, case, eng, pcm, first, n):
    """the magnitudes the pixel stage of this context works on"""
    r = case.route
    if case.kind == "render" and fused_pixels_are_mixed(r, eng):
        key = ("mixed_generic", r.name)
        if key not in g.engines:
            g.engines[key] = pixel_rows_engine(g, r, eng)
        eng = g.engines[key]
    return eng.stft_batch(pcm, first, n)


@pytest.mark.parametrize("case", fo.output_cases(), ids=lambda c: c.id)
def test_output_marks(gpu, case):
    from spectrogram_rs_amd import builtin_gradient
    g, torch = gpu, gpu.torch
    r, kind, rb = case.route, case.kind, case.row_bytes
    W, H, Cn = r.W, r.H, r.channels
    eng = g.engine(r) if case.R == fo.ROWS_DEFAULT else g.engine(r, rows=case.R)
    assert eng.R == case.R and eng.pairs == 1 and fo.out_row_bytes(r, kind, eng.R) == rb
    if kind in fo.BANK_KINDS:   # the fused kernel on the 4096-point family, the workspace and the stage kernel on the other
        fb = far_bank_of(eng)
        assert (fb.fused, fb.cross_fused) == (ba.fbank_fused(r), ba.fbank_fused(r, cross=True)) == ((1, 1) if case.family == "k1_lr" else (0, 0))
    F, rows, rw, group = case.frames, case.rows, rb // 4, case.group
    pcm = eng.white_noise(case.n_samples, seed=fo.NOISE_SEED)
    assert eng.num_frames(case.n_samples) == F
    dtype = {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}[ELEM[kind]]
    prefill, guard = ba.as_i32(ba.prefill_word(ELEM[kind], False)), ba.as_i32(ba.GUARD_WORD)
    total = rows * rw
    buf = torch.full((total + ba.guard_bytes(rb) // 4,), prefill, dtype=torch.int32, device="cuda")
    buf[total:] = guard
    payload = buf[:total]
    run(eng, kind, pcm, 0, F, out=payload.view(dtype))
    # (a) the guard is intact and no prefill is left
    assert bool((buf[total:] == guard).all()), (case.id, "the guard was written")
    left = count_equal(torch, payload, prefill)
    assert left == 0, (case.id, left, "words still hold the prefill")
    # (c) the checksum of the whole against the same frames in pieces below 2^31 bytes, each in a small buffer of its own
    whole = eng.checksum(payload)
    piece_buf = torch.empty(max(n for _, n in case.pieces()) * rw, dtype=torch.int32, device="cuda")
    pieces = 0
    for a, n in case.pieces():
        piece_buf[:n * rw] = prefill
        run(eng, kind, pcm, a * group, n * group, out=piece_buf.view(dtype))
        pieces = (pieces + eng.checksum(piece_buf[:n * rw], base_word=a * rw)) % (1 << 64)
    assert whole == pieces, (case.id, "the checksum of the whole differs from the sum over the pieces")
    del piece_buf
    if kind in fo.WELCH_KINDS:
        # group 1 is the summand itself: the whole against rn(m * m) (the four cross terms) of the engine's own rows, piece by piece --
        # rows written by direct calls, not through the workspace's ranges
        assert eng.psd_fused == 0 and eng.csd_fused == 0
        ranges = ba.welch_ranges(W, r.pairs, kind == "csd_1", F, 1, True).ranges
        assert len(ranges) >= 40 and ranges[-1].frames[1] == F > 1 << 17, (case.id, len(ranges))
        if kind == "psd_1":   # the rows launch of a full range takes the measured weights and their pool on the whole device
            n_range = ranges[0].frames[1] - ranges[0].frames[0]
            assert eng.cu_limit == torch.cuda.get_device_properties(0).multi_processor_count
            print(f"FAR-WELCH {case.id}: {len(ranges)} ranges of {n_range} frames, weights {eng.run_weights(n_range)}, claim {eng.run_claim(n_range)}")
        own = 0
        for a, n in case.pieces():
            rows_ = eng.stft_batch(pcm, a, n) if kind == "psd_1" else torch.view_as_real(eng.stft_batch_complex(pcm, a, n)).reshape(n, 1, W - 1, 4)
            x = welch_terms(torch, kind, rows_)
            del rows_
            own = (own + eng.checksum(x.view(-1).view(torch.int32), base_word=a * rw)) % (1 << 64)
            del x
        assert whole == own, (case.id, "the checksum of the whole differs from that of the summands of the engine's own rows")
    # (b) the probe rows
    sr = eng.info.sample_rate_u32
    grad = builtin_gradient("viridis")
    ends = eng.bin_edges()
    mark_rows = {m // rb for m in fo.OUTPUT_MARKS}
    worst = 0.0
    for k in case.probes():
        t0 = k * group
        first, n = t0, group
        if r.paired:   # pair-aligned: the frames of a transform stay together
            first = t0 - t0 % 2
            n = min(2, F - first)
        one = run(eng, kind, pcm, first, n)
        j = (t0 - first) // group
        row = payload[k * rw:(k + 1) * rw]
        assert torch.equal(row, words(torch, one[j])), (case.id, k, "differs from a call of that frame alone")
        if kind in ("stft", "complex"):
            host = {t: cpu_noise(r, t * H, t * H + W) for t in range(first, first + n)}
            truth = Truth(r, lambda t: host.get(t))
            got = one[j].cpu().numpy()
            ratio = truth.hold(f"{case.id} row {k}", t0, got if kind == "stft" else None, got if kind == "complex" else None)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case.id, k, ratio, "misses the float64 truth")
        elif kind in fo.WELCH_KINDS:   # the header's sum order over the engine's own rows of that frame (tests/psd_reference.py), bit for bit
            if kind == "psd_1":
                x = pr.psd_terms(eng.stft_batch(pcm, first, n).cpu().numpy())
            else:
                x = pr.csd_terms(torch.view_as_real(eng.stft_batch_complex(pcm, first, n)).cpu().numpy())
            want = pr.welch_mean(x, 1)
            assert np.array_equal(one[j].cpu().numpy().view(np.uint32), want[j].view(np.uint32)), (case.id, k, "differs from the definition over the engine's rows")
        elif kind == "fbank":   # the header's definition over the engine's own rows of that frame (tests/fbank_reference.py), bit for bit
            want = fr.bank_sums(eng.stft_batch(pcm, first, n)[j].cpu().numpy(), fo.far_bank(eng.M), 2)
            assert np.array_equal(one[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (case.id, k, "differs from the definition over the engine's rows")
        elif kind == "fbank_cross":
            spec = torch.view_as_real(eng.stft_batch_complex(pcm, first, n))[j].cpu().numpy()
            want = fr.cross_sums(spec, fo.far_bank(eng.M))
            assert np.array_equal(one[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (case.id, k, "differs from the definition over the engine's rows")
        elif kind == "render":
            mags = own_rows(g, case, eng, pcm, first, n)[j, 0].cpu().numpy()
            want = oracle.render_columns(mags[None], sr, grad, R=eng.R)[0]
            assert np.array_equal(one[j, 0].cpu().numpy(), want), (case.id, k, "differs from the oracle's pixels of the engine's rows")
        elif kind in ("bands", "peak_2") and (case.R == fo.ROWS_DEFAULT or k in mark_rows):
            # (65536 rows: the oracle's band mean is called row by row -- on the rows that hold a mark only)
            frames = range(t0, t0 + group)
            cols = []
            for t in frames:
                q = t - t % 2 if r.paired else t
                m = eng.stft_batch(pcm, q, min(2, F - q) if r.paired else 1)[t - q, 0].cpu().numpy()
                cols.append(np.stack([oracle.magnitude_in(m, sr, float(ends[py]), float(ends[py + 1])) for py in range(eng.R)]))
            want = np.maximum.reduce(cols)
            got = one[j, 0].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(got, want), \
                (case.id, k, "differs from the oracle's band means of the engine's rows")
    if kind in ("stft", "complex"):
        print(f"FAR-RATIO {case.id}: {worst:.4f} of the bound {bound_of(r)}")
        note(f"part 4 {case.family}", worst)
    del buf, payload, pcm
    torch.cuda.synchronize()


# ---- the inverse: t H and first_sample beyond 2^32 (part 3), more than 2^32 bytes of samples out (part 4) ------------------------------------
def random_spectra(r, F, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, r.pairs, r.W - 1, 2)) + 1j * rng.standard_normal((F, r.pairs, r.W - 1, 2))).astype(np.complex64)


def hold_frame_to_the_definition(y, lo, spec, t, r, win, what, eng=None, dev=None):
    """y: samples [lo, lo + len(y)) of the output, a range around frame t of non-overlapping frames: the frame against
    test_gpu_istft.definition at its bound, the gaps on either side exactly zero -- and, the compact replay, bit for bit what the same
    context makes of that frame's spectrum alone (the definition's bound is wide at the ends of a window no other frame overlaps).
    Returns the worst ratio."""
    from test_gpu_istft import check_definition, definition
    a = t * r.H - lo
    assert a >= 0 and a + r.W <= len(y), what
    if eng is not None:
        alone = eng.istft_batch(dev[t:t + 1].contiguous()).cpu().numpy()
        assert alone.shape == (r.W, r.channels)
        assert np.array_equal(alone.view(np.uint32), np.ascontiguousarray(y[a:a + r.W]).view(np.uint32)), (what, "differs from the frame alone")
    ref, env = definition(spec[t:t + 1], r.W, r.H, win, r.channels)
    assert not y[:a].any() and not y[a + r.W:].any(), (what, "a gap between two frames is not exactly zero")
    worst = check_definition(y[a:a + r.W], ref, env, r.W, r.H, win)
    assert worst <= 1.0, (what, worst, "misses the definition")
    return worst


@pytest.mark.parametrize("which", list(fo.INVERSE_ROWS))
def test_inverse_far_samples(gpu, which):
    torch = gpu.torch
    r = fo.inverse_route(which, fo.INVERSE_FAR_H)
    eng = gpu.engine(r)
    assert eng.istft_supported() == 1
    F, W, H, m = fo.INVERSE_FAR_FRAMES, r.W, r.H, fo.INVERSE_MARGIN
    spec = random_spectra(r, F, 31)
    dev = torch.from_numpy(spec).cuda()
    win = eng.window()
    N = (F - 1) * H + W
    for t in range(1, F):
        s0 = t * H - m
        y = eng.istft_batch(dev, first_sample=s0, max_samples=W + 2 * m)
        assert y.shape == (min(W + 2 * m, N - s0), r.channels)
        worst = hold_frame_to_the_definition(y.cpu().numpy(), s0, spec, t, r, win, (which, t), eng, dev)
        note(f"part 3 inverse {which}", worst)
    # a range that begins inside the gap behind frame 4, beyond sample 2^32, and holds nothing but zeros
    y = eng.istft_batch(dev, first_sample=4 * H + W + 5, max_samples=4099)
    assert y.shape == (4099, r.channels) and not bool(y.any())


@pytest.mark.parametrize("which", list(fo.INVERSE_ROWS))
def test_inverse_output_marks(gpu, which):
    torch = gpu.torch
    r = fo.inverse_route(which, fo.INVERSE_OUT_H)
    eng = gpu.engine(r)
    assert eng.istft_supported() == 1
    F, W, H, Cn, m = fo.inverse_out_frames(), r.W, r.H, r.channels, fo.INVERSE_MARGIN
    spec = random_spectra(r, F, 41)
    dev = torch.from_numpy(spec).cuda()
    win = eng.window()
    N = (F - 1) * H + W
    total = N * Cn
    assert total * 4 > 1 << 32
    prefill, guard = ba.as_i32(ba.prefill_word("f32", False)), ba.as_i32(ba.GUARD_WORD)
    buf = torch.full((total + ba.guard_bytes(Cn * 4) // 4,), prefill, dtype=torch.int32, device="cuda")
    buf[total:] = guard
    payload = buf[:total]
    y = eng.istft_batch(dev, out=payload.view(torch.float32))
    assert y.shape == (N, Cn)
    # (a)
    assert bool((buf[total:] == guard).all()), (which, "the guard was written")
    left = count_equal(torch, payload, prefill)
    assert left == 0, (which, left, "words still hold the prefill")
    # (c)
    whole = eng.checksum(payload)
    pieces = 0
    piece_buf = torch.empty(max(n for _, n in fo.sample_pieces(N, Cn)) * Cn, dtype=torch.float32, device="cuda")
    for a, n in fo.sample_pieces(N, Cn):
        piece_buf[:n * Cn] = float("inf")
        part = eng.istft_batch(dev, first_sample=a, max_samples=n, out=piece_buf)
        assert part.shape == (n, Cn)
        pieces = (pieces + eng.checksum(piece_buf[:n * Cn], base_word=a * Cn)) % (1 << 64)
    assert whole == pieces, (which, "the checksum of the whole differs from the sum over the pieces")
    del piece_buf
    # (b) the frames that hold the marks, their neighbours, the first and the last
    for t in fo.inverse_probe_frames(F):
        lo, hi = max(t * H - m, 0), min(t * H + W + m, N)
        one = eng.istft_batch(dev, first_sample=lo, max_samples=hi - lo)
        assert torch.equal(words(torch, one), payload[lo * Cn:hi * Cn]), (which, t, "differs from a call of that range alone")
        worst = hold_frame_to_the_definition(one.cpu().numpy(), lo, spec, t, r, win, (which, t), eng, dev)
        note(f"part 4 inverse {which}", worst)
    # every sample outside the frames is an exact zero: as many non-zero words as the frames can hold at the most
    nonzero = sum(int((payload[a:a + SLICE_WORDS] != 0).sum()) for a in range(0, total, SLICE_WORDS))
    assert nonzero <= F * W * Cn, (which, nonzero)
    del buf, payload
    torch.cuda.synchronize()


# ---- part 4, the stand-alone pixel stage: sgx_render_mags, sgx_magnitude_in, sgx_render_bands with input and output past 2^32 bytes ------
ORACLE_RANGES = 1024   # the most ranges of one column the oracle's band mean is called on: evenly spaced, the first and the last among them


def pixel_ranges(n):
    edges = np.geomspace(32.0, 20000.0, n + 1)
    return np.stack([edges[:-1], edges[1:]], 1).astype(np.float32)


def lds_optin(torch):
    """the LDS a workgroup of this device may ask for (hipDeviceAttributeSharedMemPerBlockOptin), which the launchers compare with.  torch
    does not show it: the runtime is asked, and the attribute before it in the same enumeration is held to the figure torch does show"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    per_block, optin = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(per_block), 74, 0) == 0 and hip.hipDeviceGetAttribute(ctypes.byref(optin), 75, 0) == 0
    assert per_block.value == torch.cuda.get_device_properties(0).shared_memory_per_block, per_block.value
    assert optin.value >= per_block.value
    return optin.value


def pixel_call(eng, case, src, out=None):
    if case.entry == "render_mags":
        return eng.render_mags(src, out=out)
    if case.entry == "render_bands":
        return eng.render_bands(src, out=out)
    return eng.magnitude_in(src, pixel_ranges(case.n_ranges), out=out)


@pytest.mark.parametrize("case", fo.PIXEL_CASES, ids=lambda c: c.id)
def test_pixel_stage_marks(gpu, case):
    from pixel_plans import ramp
    from spectrogram_rs_amd import SpectrogramEngine, builtin_gradient
    g, torch = gpu, gpu.torch
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", window_samples=case.W, hop_samples=max(case.W // 2, 1), channels=2,
                            rows=case.R, large_transforms=case.large)
    try:
        grad = builtin_gradient("viridis")
        if case.n_lut != 256:
            grad = ramp(case.n_lut)
            eng.set_gradient(grad)
        assert (eng.W, eng.R, eng.M, len(grad)) == (case.W, case.R, case.W - 1, case.n_lut)
        # the kernel body this context takes, from the launchers' own quantities as this device and this context have them
        cap = min(lds_optin(torch), 160 << 10)
        body = fo.pixel_body(case.entry, eng.M, eng.info.total_samples_per_column, case.n_lut, cap)
        print(f"FAR-BODY {case.id}: {body} (LDS cap {cap}, {eng.info.total_samples_per_column} samples per column, {case.n_lut} palette entries)")
        assert body == case.body, (case.id, body, cap)
        run_pixel_case(g, case, eng, grad)
    finally:
        torch.cuda.synchronize()
        eng.close()


def run_pixel_case(g, case, eng, grad):
    torch = g.torch
    cols, entry = case.cols, case.entry
    iw, ow = case.in_col_bytes // 4, case.out_col_bytes // 4
    assert iw == (eng.R if entry == "render_bands" else eng.M) * 2
    # magnitudes from 1e-7 to 1: squares of the engine's noise, written in place
    src = eng.white_noise(cols * iw, seed=fo.NOISE_SEED, channels=1)
    src.mul_(src).add_(1e-7)
    src_cols = src.view(cols, iw // 2, 2)
    before = eng.checksum(src)
    elem = "f32" if entry == "magnitude_in" else "u8"
    dtype = torch.float32 if elem == "f32" else torch.uint8
    prefill, guard = ba.as_i32(ba.prefill_word(elem, False)), ba.as_i32(ba.GUARD_WORD)
    total = cols * ow
    buf = torch.full((total + ba.guard_bytes(case.out_col_bytes) // 4,), prefill, dtype=torch.int32, device="cuda")
    buf[total:] = guard
    payload = buf[:total]
    pixel_call(eng, case, src_cols, out=payload.view(dtype))
    # (a)
    assert bool((buf[total:] == guard).all()), (case.id, "the guard was written")
    left = count_equal(torch, payload, prefill)
    assert left == 0, (case.id, left, "words still hold the prefill")
    assert eng.checksum(src) == before, (case.id, "the input was written")
    # (c) pieces of columns below 2^31 bytes on either side, each from a small copy of its input into a small buffer
    whole = eng.checksum(payload)
    per = max(n for _, n in case.pieces())
    piece_in = torch.empty(per * iw, dtype=torch.float32, device="cuda")
    piece_out = torch.empty(per * ow, dtype=torch.int32, device="cuda")
    pieces = 0
    for a, n in case.pieces():
        piece_in[:n * iw] = src[a * iw:(a + n) * iw]
        piece_out[:n * ow] = prefill
        pixel_call(eng, case, piece_in[:n * iw].view(n, iw // 2, 2), out=piece_out.view(dtype))
        pieces = (pieces + eng.checksum(piece_out[:n * ow], base_word=a * ow)) % (1 << 64)
    assert whole == pieces, (case.id, "the checksum of the whole differs from the sum over the pieces")
    del piece_in, piece_out
    # (b) the columns that hold a mark of the input or of the output, their neighbours, the first and the last
    sr = eng.info.sample_rate_u32
    ranges = pixel_ranges(case.n_ranges)
    picked = np.unique(np.linspace(0, case.n_ranges - 1, min(case.n_ranges, ORACLE_RANGES)).round().astype(int))
    for k in case.probes():
        col = src_cols[k:k + 1].clone()
        one = pixel_call(eng, case, col)
        assert torch.equal(words(torch, one), payload[k * ow:(k + 1) * ow]), (case.id, k, "differs from a call of that column alone")
        host = col[0].cpu().numpy()
        if entry == "render_mags":
            want = oracle.render_columns(host[None], sr, grad, R=eng.R)[0]
            assert np.array_equal(one[0].cpu().numpy(), want), (case.id, k, "differs from the oracle's pixels")
        elif entry == "magnitude_in":
            want = np.stack([oracle.magnitude_in(host, sr, float(f0), float(f1)) for f0, f1 in ranges[picked]])
            assert np.array_equal(one[0].cpu().numpy()[picked].view(np.uint32), want.view(np.uint32)), (case.id, k, "differs from the oracle's band means")
    del buf, payload, src, src_cols
    torch.cuda.synchronize()


# ---- part 4, the filterbank stages alone: sgx_fbank_mags, sgx_fbank_cross_spec with an output past 2^32 bytes -----------------------------
@pytest.mark.parametrize("case", fo.BANK_STAGE_CASES, ids=lambda c: c.id)
def test_bank_stage_marks(gpu, case):
    """the stage kernels place a column's sums at `col * n_filters`: with 1024 filters the element index passes 2^28 and 2^29 (bytes 2^31 and
    2^32) at columns the case probes.  The guard, the prefill, the checksum in pieces, and the probe columns against the header's definition
    (tests/fbank_reference.py) bit for bit"""
    from spectrogram_rs_amd import SpectrogramEngine
    g, torch = gpu, gpu.torch
    eng = SpectrogramEngine(es.SR, device=0, window_samples=case.W, hop_samples=case.W // 2, channels=2)
    try:
        assert eng.M == case.M
        bank = fo.far_bank(eng.M)
        fb = eng.filterbank(*bank, power=2)
        cross = case.entry == "fbank_cross_spec"
        cols, iw, ow = case.cols, case.in_col_bytes // 4, case.out_col_bytes // 4
        call = (lambda src, out=None: fb.cross_apply(src.view(-1, eng.M, 2, 2), out=out)) if cross else \
            (lambda src, out=None: fb.apply(src.view(-1, eng.M, 2), out=out))
        # the engine's noise as it is for the complex rows (either sign), its squares plus 1e-7 as magnitudes
        src = eng.white_noise(cols * iw, seed=fo.NOISE_SEED, channels=1)
        if not cross:
            src.mul_(src).add_(1e-7)
        before = eng.checksum(src)
        prefill, guard = ba.as_i32(ba.prefill_word("f32", False)), ba.as_i32(ba.GUARD_WORD)
        total = cols * ow
        buf = torch.full((total + ba.guard_bytes(case.out_col_bytes) // 4,), prefill, dtype=torch.int32, device="cuda")
        buf[total:] = guard
        payload = buf[:total]
        call(src, out=payload.view(torch.float32))
        # (a)
        assert bool((buf[total:] == guard).all()), (case.id, "the guard was written")
        left = count_equal(torch, payload, prefill)
        assert left == 0, (case.id, left, "words still hold the prefill")
        assert eng.checksum(src) == before, (case.id, "the input was written")
        # (c) pieces of columns below 2^31 bytes of output, each into a small buffer of its own
        whole = eng.checksum(payload)
        per = max(n for _, n in case.pieces())
        piece_out = torch.empty(per * ow, dtype=torch.int32, device="cuda")
        pieces = 0
        for a, n in case.pieces():
            piece_out[:n * ow] = prefill
            call(src[a * iw:(a + n) * iw], out=piece_out.view(torch.float32))
            pieces = (pieces + eng.checksum(piece_out[:n * ow], base_word=a * ow)) % (1 << 64)
        assert whole == pieces, (case.id, "the checksum of the whole differs from the sum over the pieces")
        del piece_out
        # (b) the columns whose sums hold a mark, their neighbours, the first and the last
        for k in case.probes():
            col = src[k * iw:(k + 1) * iw].clone()
            one = call(col)
            assert torch.equal(words(torch, one), payload[k * ow:(k + 1) * ow]), (case.id, k, "differs from a call of that column alone")
            host = col.cpu().numpy()
            want = fr.cross_sums(host.reshape(1, eng.M, 2, 2), bank) if cross else fr.bank_sums(host.reshape(1, eng.M, 2), bank, 2)
            assert np.array_equal(one.cpu().numpy().view(np.uint32), want.view(np.uint32)), (case.id, k, "differs from the definition")
        del buf, payload, src
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- part 4, the Welch stages alone: sgx_psd_mags, sgx_csd_spec with input and output past 2^32 bytes -------------------------------------
@pytest.mark.parametrize("case", fo.WELCH_STAGE_CASES, ids=lambda c: c.id)
def test_welch_stage_marks(gpu, case):
    """The block kernel reads frame f of element e at `f * elems + e` and the combine writes column j at `j * elems + e`: with rows of 63
    bins both indices pass bytes 2^31 and 2^32 at frames and columns the case probes.  Group 1: the output crosses the marks the input
    crosses.  Group 2: the output crosses 2^31 only, and input frame 2 j + 1 of the columns behind it lies past both marks.  The guard, the
    prefill, the checksum of the whole against that of a torch expression over the same input in pieces, and the probe columns against
    the header's sum order (tests/psd_reference.py) over the same input rows fetched from the device, bit for bit"""
    from spectrogram_rs_amd import SpectrogramEngine
    g, torch = gpu, gpu.torch
    eng = SpectrogramEngine(es.SR, device=0, window_samples=case.W, hop_samples=case.W // 2, channels=2)
    try:
        assert eng.M == case.M and eng.pairs == 1 and eng.psd_fused == 0 and eng.csd_fused == 0
        cross = case.entry == "csd_spec"
        comps = 4 if cross else 2
        F, rw = case.frames, case.row_bytes // 4
        assert rw == eng.M * comps
        stage = eng.csd_spec if cross else eng.psd_mags
        terms = pr.csd_terms if cross else pr.psd_terms
        # the engine's noise as it is for the complex rows (either sign), its squares plus 1e-7 as magnitudes
        src = eng.white_noise(F * rw, seed=fo.NOISE_SEED, channels=1)
        if not cross:
            src.mul_(src).add_(1e-7)
        rows = src.view(F, 1, eng.M, 2, 2) if cross else src.view(F, 1, eng.M, 2)
        before = eng.checksum(src)
        prefill, guard = ba.as_i32(ba.prefill_word("f32", False)), ba.as_i32(ba.GUARD_WORD)
        for group in case.groups:
            cols = case.cols(group)
            marks_in, marks_out = case.crossed(group)
            assert marks_in == fo.OUTPUT_MARKS and marks_out == fo.OUTPUT_MARKS[:3 - group], (case.id, group)
            total = cols * rw
            buf = torch.full((total + ba.guard_bytes(case.row_bytes) // 4,), prefill, dtype=torch.int32, device="cuda")
            buf[total:] = guard
            payload = buf[:total]
            got = stage(rows, group, out=payload.view(torch.float32))
            assert got.data_ptr() == payload.data_ptr()
            # (a)
            assert bool((buf[total:] == guard).all()), (case.id, group, "the guard was written")
            left = count_equal(torch, payload, prefill)
            assert left == 0, (case.id, group, left, "words still hold the prefill")
            assert eng.checksum(src) == before, (case.id, group, "the input was written")
            # (c) the whole against the torch expression over the same input, in pieces below 2^31 bytes of input and of output
            whole, expr = eng.checksum(payload), 0
            for a, n in case.pieces(group):
                f0, f1 = a * group, min((a + n) * group, F)
                x = welch_terms(torch, case.entry, src[f0 * rw:f1 * rw].view(f1 - f0, eng.M, comps))
                if group == 2:
                    x = welch_means_of_two(torch, x)
                assert x.shape[0] == n and x.numel() * 4 < fo.PIECE_LIMIT
                expr = (expr + eng.checksum(x.view(-1).view(torch.int32), base_word=a * rw)) % (1 << 64)
                del x
            assert whole == expr, (case.id, group, "the checksum of the whole differs from that of the torch expression over the input")
            # (b) the columns that hold a mark of the output or whose frames hold a mark of the input, their neighbours, the first, the last
            for k in case.probes(group):
                f0, f1 = k * group, min((k + 1) * group, F)
                host = rows[f0:f1].cpu().numpy()
                want = pr.welch_mean(terms(host), group)
                assert want.shape[0] == 1
                assert np.array_equal(payload[k * rw:(k + 1) * rw].cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32)), \
                    (case.id, group, k, "differs from the definition over the same rows")
                one = stage(rows[f0:f1].clone(), group)
                assert torch.equal(words(torch, one), payload[k * rw:(k + 1) * rw]), (case.id, group, k, "differs from a call of that column alone")
            del buf, payload, got
        del src, rows
    finally:
        torch.cuda.synchronize()
        eng.close()

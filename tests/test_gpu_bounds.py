"""Where the batch entry points read and write: every route of tests/edge_signals.py:ROUTES with its buffers inside guarded arenas
(tests/bounds_arena.py), all through SpectrogramEngine and the C ABI.

The tuned kernels address the stream and the rows through buffer descriptors whose record counts do the clipping; a count that is one
frame, one channel or one row too generous gives correct results wherever the caller allocates exactly what the call needs.  Here
  A  every output lies between two guards, prefilled with +inf and then with all ones, at 16-byte and at 8-modulo-16 alignment: the
     payload must hold the bits of a clean run, both guards must be untouched and no prefill may survive;
  B  the stream lies inside a NaN arena and every sample outside the ones the requested frames own is NaN as well;
  C  one context runs every entry point on an overflowing and on an all-NaN stream before the real one (workspace, partial peak
     columns, kernel 11's scratch, the inverse's tables);
  D  the pixel-stage entry points (render_mags, render_bands, magnitude_in) get the same arenas;
  E  the chunk loops over the 192 MiB workspace are crossed, a peak column accumulating over several chunks included.
The filterbank calls (sgx_fbank_batch, sgx_fbank_cross_batch; the stages sgx_fbank_mags, sgx_fbank_cross_spec under D) run through all of
it with one bank per context, fbank_reference.edge_bank at power 2: their baselines equal the stage over the baseline's own rows and, on
three frames, the header's definition as tests/fbank_reference.py computes it, bit for bit.  sgx_fbank_cross_batch asks for 16 bytes: its
8-modulo-16 variant asserts the refusal and an untouched arena.
The Welch calls (sgx_psd_batch, sgx_csd_batch at groups 1, 3 and n + 5; the stages sgx_psd_mags, sgx_csd_spec under D) run through all of
it as well: their baseline is the header's sum order (tests/psd_reference.py) over the baseline's own rows of the requested sub-range,
bit for bit, the columns counted from the sub-range's first frame; sgx_csd_batch asks for 16 bytes like the cross sums.  Under E the
seams of psd_reduce's ranges that bounds_arena.welch_ranges selects: a carried column off kernel 11, a seam on an odd frame of a paired
context.
All of it is bit for bit against a clean baseline (the whole stream through a fresh engine on fresh, exact-size tensors), and the
baseline's rows are held to the float64 truth on three frames at the bound the project holds white noise to.  No skips: a (row, entry
point) pair is left out only through EXPECTED_UNSUPPORTED, and the library must refuse exactly those.  Run with -m gpu on an MI355X."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import bounds_arena as ba
import edge_signals as es
import fbank_reference as fr
import oracle
import psd_reference as pr
from conftest import chirpz_bound, mags_error
from spectrogram_rs_amd import SpectrogramEngine, _lib
from test_gpu_peak import amax_groups, same

pytestmark = pytest.mark.gpu

ROWS = [r.name for r in es.ROUTES]
VARIANTS = ["aligned", "odd"]
WELCH_KINDS = ["psd_1", "psd_3", "psd_n5", "csd_3", "csd_n5"]   # the groups of the peak kinds: 1, 3, and n + 5 for one short column
KINDS = ["stft", "f16", "complex", "render", "bands", "peak_1", "peak_3", "peak_n", "peak_n5", "fbank", "fbank_cross"] + WELCH_KINDS
ELEM = {"stft": "f32", "f16": "f16", "complex": "f32", "render": "u8", "bands": "f32", "istft": "f32", "magnitude_in": "f32",
        "render_mags": "u8", "render_bands": "u8", "fbank": "f32", "fbank_cross": "f32", "fbank_mags": "f32", "fbank_cross_spec": "f32",
        "psd_1": "f32", "psd_3": "f32", "psd_n5": "f32", "csd_3": "f32", "csd_n5": "f32", "psd_mags": "f32", "csd_spec": "f32"}
# the only (row, entry point) pairs this file leaves out: the library must answer SGX_ERR_UNSUPPORTED / istft_supported() == 0 for
# exactly these (test_expected_unsupported), any other refusal fails the test that meets it
EXPECTED_UNSUPPORTED = ({(r.name, "istft") for r in es.ROUTES if r.kernel == 11} | {(r.name, "fbank_cross") for r in es.ROUTES if r.channels == 1}
                        | {(r.name, k) for r in es.ROUTES if r.channels == 1 for k in WELCH_KINDS if k.startswith("csd")})
INVERSE_ROWS = [n for n in ROWS if (n, "istft") not in EXPECTED_UNSUPPORTED]
SERVED = [(n, k) for k in KINDS for n in ROWS if (n, k) not in EXPECTED_UNSUPPORTED]      # (row, kind) of the sweeps over KINDS


def kinds_of(name):
    return [k for k in KINDS if (name, k) not in EXPECTED_UNSUPPORTED]


# the rows whose column of magnitudes no LDS holds ((M + 1) * 8 bytes against the 160 KB of a workgroup): the pixel and bands stages read
# them from global memory, in instantiations of their own (render_kernel<false>, magnitude_in_kernel<false>)
# (the launchers compare with min(the device's opt-in LDS, 160 KB), and launch_render adds its threshold tables, (n_lut + 255) * 4
# bytes -- about 2 KB with a built-in gradient -- to the column first.  So a row whose column lies within UNSTAGED_TABLES_MARGIN below
# the limit may go either way and must not be added to ROUTES without deriving this list anew: test_unstaged_rows_are_the_long_windows
# fails on one.)
UNSTAGED_TABLES_MARGIN = 8 << 10
UNSTAGED_ROWS = [r.name for r in es.ROUTES if r.W * 8 > 160 << 10]
_cache = {}


@pytest.fixture(scope="module")
def torch_cuda():
    """torch, and the end of this module's engines: the cases built on the way (45 engines with their streams and baselines, the W 2^20
    row among them) are closed and dropped before the next test file runs"""
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    yield torch
    torch.cuda.synchronize()
    for v in _cache.values():
        (v.eng if isinstance(v, SimpleNamespace) else v).close()
    _cache.clear()
    torch.cuda.empty_cache()


def engine(r, **extra):
    return SpectrogramEngine(es.SR, device=0, **r.engine_kwargs(), **extra)


def elem_of(kind):
    return ELEM["bands" if kind.startswith("peak") else kind]


def dtype_of(torch, kind):
    return {"f32": torch.float32, "f16": torch.float16, "u8": torch.uint8}[elem_of(kind)]


def welch(kind):
    """"psd" or "csd" of a Welch kind, None of any other"""
    return kind[:3] if kind in WELCH_KINDS else None


def group_of(kind, n):
    return {"1": 1, "3": 3, "n": n, "n5": n + 5}[kind.split("_")[1]]


def rows_of(kind, n):
    return -(-n // group_of(kind, n)) if kind.startswith("peak") or welch(kind) else n


def bank_of(eng):
    """the engine's bank of the sweep, made once per context: fbank_reference.edge_bank over its bins, power 2"""
    if getattr(eng, "_bounds_bank", None) is None:
        eng._bounds_bank = eng.filterbank(*fr.edge_bank(eng.M), power=2)
        assert eng._bounds_bank.n_filters == ba.N_BANK_FILTERS
    return eng._bounds_bank


def row_bytes(eng, kind):
    if kind in ("fbank", "fbank_cross"):
        return eng.pairs * ba.N_BANK_FILTERS * (8 if kind == "fbank" else 16)
    if kind in ("stft", "f16", "complex"):
        return eng.pairs * eng.M * {"stft": 8, "f16": 4, "complex": 16}[kind]
    if welch(kind) or kind in ("psd_mags", "csd_spec"):
        return eng.pairs * eng.M * (8 if kind.startswith("psd") else 16)
    return eng.pairs * eng.R * (4 if kind == "render" else 8)


def run(eng, kind, dev, first, n, out=None):
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
    if welch(kind):
        return (eng.psd_batch if welch(kind) == "psd" else eng.csd_batch)(dev, group_of(kind, n), first, n, out=out)
    return eng.bands_peak_batch(dev, group_of(kind, n), first, n, out=out)


def words(torch, t):
    """any result as flat int32 words"""
    if t.dtype == torch.complex64:
        t = torch.view_as_real(t)
    return t.contiguous().view(-1).view(torch.int32)


class Arena:
    """[front guard | payload | back guard] in one int32 allocation (bounds_arena.layout); `guard` fills both guards, `fill` the payload"""

    def __init__(self, torch, payload_bytes, row_bytes_, odd, fill, guard=ba.GUARD_WORD, mod4=False):
        slack = 16
        self.torch, self.guard = torch, ba.as_i32(guard)
        self.words = torch.full(((2 * ba.guard_bytes(row_bytes_) + payload_bytes + slack) // 4,), self.guard, dtype=torch.int32, device="cuda")
        base = self.words.data_ptr()
        assert base % 8 == 0
        lay = ba.layout(payload_bytes, row_bytes_, odd, base % 16, mod4=mod4)
        assert lay.total_bytes <= self.words.numel() * 4
        self.lo, self.hi = lay.payload_offset // 4, lay.back_offset // 4
        self.words[self.lo:self.hi] = ba.as_i32(fill)
        at = base + lay.payload_offset
        assert at % 8 == 4 if mod4 else at % 16 == (8 if odd else 0), "the payload is not where the variant puts it"

    def payload(self, dtype=None):
        p = self.words[self.lo:self.hi]
        return p if dtype is None else p.view(dtype)

    def guards_intact(self):
        return bool((self.words[:self.lo] == self.guard).all()) and bool((self.words[self.hi:] == self.guard).all())


def to_dev(torch, r, pcm):
    """a fresh, exact-size stream (the align4 row: 4 but not 8 bytes aligned, as tests/test_gpu_edges.py places it)"""
    flat = torch.from_numpy(np.ascontiguousarray(pcm, np.float32).reshape(-1)).cuda()
    if not r.align4:
        return flat
    buf = torch.zeros(flat.numel() + 1, dtype=torch.float32, device="cuda")
    buf[1:] = flat
    assert buf[1:].data_ptr() % 8 == 4
    return buf[1:]


def frames_of(r):
    return 5 if r.W >= 65536 else max(9, r.min_frames)


def case(torch, name):
    """The row's engine (its kernel and render_path bits asserted first, as tests/test_gpu_edges.py::test_route does), its noise stream
    and the clean baseline of every entry point, built once and never changed."""
    if name in _cache:
        return _cache[name]
    r = es.ROUTE[name]
    eng = engine(r, gradient="viridis")
    info = eng.info
    assert info.stft_kernel == r.kernel, (name, info.stft_kernel)
    assert info.render_path & r.bits_set == r.bits_set and info.render_path & r.bits_clear == 0, (name, info.render_path)
    if r.bands_fused is not None:
        assert eng.bands_fused == r.bands_fused, (name, eng.bands_fused)
    W, H, Cn = r.W, r.H, r.channels
    F = frames_of(r)
    N = (F - 1) * H + W
    pcm = (oracle.white_noise(N * Cn, seed=0x5EED0900 + ROWS.index(name)) * np.float32(0.25)).reshape(N, Cn)
    dev = to_dev(torch, r, pcm)
    cs = SimpleNamespace(r=r, eng=eng, F=F, N=N, pcm=pcm, dev=dev, base={}, flat={}, terms={}, welch={})
    assert eng.psd_fused == 0 and eng.csd_fused == 0
    fb = bank_of(eng)
    assert (fb.fused, fb.cross_fused) == (ba.fbank_fused(r), ba.fbank_fused(r, cross=True)), (name, fb.fused, fb.cross_fused)
    for kind in ("stft", "f16", "complex", "render", "bands", "fbank", "fbank_cross"):
        if (name, kind) in EXPECTED_UNSUPPORTED:
            continue
        cs.base[kind] = run(eng, kind, dev, 0, F)
        cs.flat[kind] = words(torch, cs.base[kind])
        assert cs.base[kind].shape[0] == F
    anchor_banks(torch, cs, fb)
    # the anchor of every bit-identity below: the baseline's rows against the float64 truth on the first, the middle and the last frame
    got = cs.base["stft"].cpu().numpy()
    bound = chirpz_bound(W) if r.kernel == 4 else 1.0
    for t in (0, F // 2, F - 1):
        for p in range(r.pairs):
            ref = es.truth_frame(es.frame_lr(pcm[t * H:t * H + W], p), W)
            if r.paired:   # (two frames of one transform: against the pair's peak, include/sgx.h)
                q = t ^ 1
                partner = float(np.abs(es.truth_frame(es.frame_lr(pcm[q * H:q * H + W], p), W)).max()) if q < F else 0.0
                err = es.pair_error(got[t, p], ref, r.floor, partner)
            else:
                err = mags_error(got[t, p], ref, r.floor)
            assert err <= bound, (name, t, p, err, "the baseline itself misses the float64 truth")
    # the inverse, where the library serves it
    cs.istft = eng.istft_supported()
    assert (cs.istft == 0) == ((name, "istft") in EXPECTED_UNSUPPORTED), (name, cs.istft)
    if cs.istft:
        cs.spec = torch.view_as_real(cs.base["complex"]).contiguous()
        cs.base["istft"] = eng.istft_batch(cs.spec).clone()
        assert cs.base["istft"].shape == (N, Cn)
        cs.flat["istft"] = words(torch, cs.base["istft"])
    # a second copy of the stream with the longest ragged tail (H - 1 samples that belong to no frame) for the output-side families
    tail = (oracle.white_noise((H - 1) * Cn, seed=77) * np.float32(0.25)).reshape(H - 1, Cn)
    cs.dev_ragged = to_dev(torch, r, np.concatenate([pcm, tail], 0))
    torch.cuda.synchronize()
    _cache[name] = cs
    return cs


def anchor_banks(torch, cs, fb):
    """The anchor of the bank kinds: the baseline equals the stage over the baseline's own rows bit for bit, and on the first, the middle
    and the last frame (all three on every row: the W 2^20 row's take about two seconds of CPU per kind) the header's definition as
    tests/fbank_reference.py computes it, bit for bit."""
    eng, F, name = cs.eng, cs.F, cs.r.name
    bank = fr.edge_bank(eng.M)
    probe = [0, F // 2, F - 1]
    rows = cs.base["stft"]
    assert torch.equal(words(torch, fb.apply(rows.reshape(-1, eng.M, 2))), cs.flat["fbank"]), (name, "sgx_fbank_batch differs from sgx_fbank_mags of the rows")
    want = fr.bank_sums(rows[probe].cpu().numpy(), bank, 2)
    got = cs.base["fbank"][probe].cpu().numpy()
    assert got.shape == want.shape == (3, eng.pairs, ba.N_BANK_FILTERS, 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, "sgx_fbank_batch differs from the definition")
    if "fbank_cross" not in cs.base:
        return
    spec = torch.view_as_real(cs.base["complex"]).contiguous()
    assert torch.equal(words(torch, fb.cross_apply(spec.reshape(-1, eng.M, 2, 2))), cs.flat["fbank_cross"]), (name, "sgx_fbank_cross_batch differs from sgx_fbank_cross_spec of the rows")
    want = fr.cross_sums(spec[probe].cpu().numpy(), bank)
    got = cs.base["fbank_cross"][probe].cpu().numpy()
    assert got.shape == want.shape == (3, eng.pairs, ba.N_BANK_FILTERS, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, "sgx_fbank_cross_batch differs from the definition")


def calls_of(cs):
    F = cs.F
    calls = [(0, F), (0, 1), (1, 1), (1, F - 1), (2, 3), (F - 1, 1)]
    if cs.r.chunk_targets:   # one range straddling each frame next to a scratch-chunk boundary of the full run
        for b in es.chunk_boundary_frames(cs.r.W, cs.r.pairs, F):
            first = max(b - 1, 0)
            calls.append((first, min(3, F - first)))
    return calls


def want_peak(cs, kind, first, n):
    bands = cs.base["bands"][first:first + n]
    g = group_of(kind, n)
    return bands if g == 1 else amax_groups(bands, g)


def want_welch(torch, cs, kind, first, n):
    """The Welch kinds' baseline: the header's sum order (tests/psd_reference.py) over the baseline's own stft / complex rows of frames
    [first, first + n), the columns counted from `first`: flat int32 words on the device.  The summands of a row are formed once and the
    means of a (kind, first, n) once, on the host; neither is written to afterwards."""
    which = welch(kind)
    if which not in cs.terms:
        if which == "psd":
            cs.terms[which] = pr.psd_terms(cs.base["stft"].cpu().numpy())
        else:
            cs.terms[which] = pr.csd_terms(torch.view_as_real(cs.base["complex"]).cpu().numpy())
        cs.terms[which].setflags(write=False)
    key = (kind, first, n)
    if key not in cs.welch:
        cs.welch[key] = pr.welch_mean(cs.terms[which][first:first + n], group_of(kind, n)).reshape(-1).view(np.int32)
        cs.welch[key].setflags(write=False)
    return torch.tensor(cs.welch[key], device="cuda")     # (a copy: the cached means stay read-only)


def check_result(torch, cs, kind, first, n, got_words, what):
    """got_words (flat int32) against the baseline's rows [first, first + n): bit for bit; peak columns with test_gpu_peak.same against
    amax_groups of the baseline bands; the Welch kinds against want_welch"""
    if welch(kind):
        want = want_welch(torch, cs, kind, first, n)
        assert got_words.numel() == want.numel() == rows_of(kind, n) * row_bytes(cs.eng, kind) // 4, what
        assert torch.equal(got_words, want), what
    elif kind.startswith("peak"):
        want = want_peak(cs, kind, first, n)
        assert got_words.numel() == want.numel(), what
        assert same(got_words.view(torch.float32), want), what
    else:
        rw = row_bytes(cs.eng, kind) // 4
        assert torch.equal(got_words, cs.flat[kind][first * rw:(first + n) * rw]), what


def check_arena(arena, prefill, what):
    assert arena.guards_intact(), (what, "a guard was written")
    assert not bool((arena.payload() == ba.as_i32(prefill)).any()), (what, "a payload word still holds the prefill")


def test_expected_unsupported(torch_cuda):
    torch = torch_cuda
    assert {k for _, k in EXPECTED_UNSUPPORTED} == {"istft", "fbank_cross", "csd_3", "csd_n5"}
    mono = {r.name for r in es.ROUTES if r.channels == 1}
    assert all({n for n, k in EXPECTED_UNSUPPORTED if k == kind} == mono for kind in ("fbank_cross", "csd_3", "csd_n5"))
    for name in ROWS:
        cs = case(torch, name)
        for kind in ("csd_3", "csd_n5"):
            if (name, kind) not in EXPECTED_UNSUPPORTED:
                assert kind in kinds_of(name) and "complex" in cs.base, name
                continue
            # a mono context has no (l, r) pair: refused, the count zero, the buffer as it was
            out = torch.zeros(cs.F * row_bytes(cs.eng, kind) // 4, dtype=torch.float32, device="cuda")
            got = C.c_size_t(99)
            rc = cs.eng._lib.sgx_csd_batch(cs.eng._ctx, C.c_void_p(cs.dev.data_ptr()), cs.N, 0, cs.F, group_of(kind, cs.F), C.c_void_p(out.data_ptr()),
                                           C.byref(got))
            assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0, (name, kind, rc)
            assert b"sgx_csd_batch" in cs.eng._lib.sgx_last_error(cs.eng._ctx)
            torch.cuda.synchronize()
            assert not bool(out.any()), (name, kind)
        if (name, "fbank_cross") in EXPECTED_UNSUPPORTED:   # a mono context: refused, the count zero, the buffer as it was
            fb = bank_of(cs.eng)
            assert fb.cross_fused == 0
            out = torch.zeros(cs.F * row_bytes(cs.eng, "fbank_cross") // 4, dtype=torch.float32, device="cuda")
            got = C.c_size_t(99)
            rc = cs.eng._lib.sgx_fbank_cross_batch(fb._h, C.c_void_p(cs.dev.data_ptr()), cs.N, 0, cs.F, C.c_void_p(out.data_ptr()), C.byref(got))
            assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0, (name, rc)
            torch.cuda.synchronize()
            assert not bool(out.any())
        else:
            assert "fbank_cross" in cs.base, name
        if (name, "istft") not in EXPECTED_UNSUPPORTED:
            continue
        cs = case(torch, name)
        assert cs.istft == 0
        spec = torch.view_as_real(cs.base["complex"]).contiguous()
        out = torch.zeros(cs.N * cs.r.channels, dtype=torch.float32, device="cuda")
        got = C.c_size_t(99)
        rc = cs.eng._lib.sgx_istft_batch(cs.eng._ctx, C.c_void_p(spec.data_ptr()), cs.F, 0, cs.N, C.c_void_p(out.data_ptr()), C.byref(got))
        assert rc == _lib.SGX_ERR_UNSUPPORTED and got.value == 0, (name, rc)
        assert not bool(out.any())


def test_unstaged_rows_are_the_long_windows():
    assert UNSTAGED_ROWS == ["large_w1m_lr", "large_w65537_chirp_lr"]
    # every other row is staged by both launchers, the tables of launch_render included: none lies in the margin below the limit
    assert max(r.W for r in es.ROUTES if r.name not in UNSTAGED_ROWS) * 8 <= (160 << 10) - UNSTAGED_TABLES_MARGIN


@pytest.mark.parametrize("name", UNSTAGED_ROWS)
def test_unstaged_pixel_stage_against_the_oracle(torch_cuda, name):
    """The baselines of render_batch and bands_batch on these rows come from the kernels that read the column from global memory, and
    every arena run is compared with those baselines: here they, and render_mags / magnitude_in of the engine's own rows, are held to
    the CPU oracle's pixel stage over those rows, bit for bit (as tests/test_gpu_large.py and tests/test_gpu_bands.py do where the column
    fits in LDS)."""
    torch = torch_cuda
    from spectrogram_rs_amd import builtin_gradient
    cs = case(torch, name)
    eng, F = cs.eng, cs.F
    assert eng.pairs == 1 and eng.info.render_path & 1 == 0 and eng.bands_fused == 0
    sr = eng.info.sample_rate_u32
    mags = cs.base["stft"][:, 0].contiguous()          # [F][M][2]
    rows = mags.cpu().numpy()
    # pixels: render_batch's column, render_mags of the engine's rows, the oracle's pixels of them
    own = eng.render_mags(mags).cpu().numpy()
    assert np.array_equal(cs.base["render"].cpu().numpy()[:, 0], own), (name, "render_batch differs from render_mags of stft_batch's rows")
    want = oracle.render_columns(rows, sr, builtin_gradient("viridis"), R=eng.R)
    assert np.array_equal(own, want), (name, "render_mags differs from the oracle")
    # bands: bands_batch's column, magnitude_in of the engine's rows over the row ranges, the oracle's means of them
    ends = eng.bin_edges()
    got = eng.magnitude_in(mags, np.stack([ends[:-1], ends[1:]], 1)).cpu().numpy().reshape(F, eng.R, 2)
    assert np.array_equal(cs.base["bands"].cpu().numpy()[:, 0].view(np.uint32), got.view(np.uint32)), (name, "bands_batch differs from magnitude_in")
    for t in range(F):
        ref = np.stack([oracle.magnitude_in(rows[t], sr, float(ends[py]), float(ends[py + 1])) for py in range(eng.R)])
        assert np.array_equal(got[t].view(np.uint32), ref.view(np.uint32)), (name, t, "magnitude_in differs from the oracle")


# ---- A: output guards ---------------------------------------------------------------------------------------------------------------
def refused_for_alignment(torch, cs, kind, arena, first, n, what):
    """sgx_fbank_cross_batch and sgx_csd_batch want 16 bytes (include/sgx.h): at 8 modulo 16 they answer SGX_ERR_INVALID_ARG and write
    nothing"""
    before = arena.words.clone()
    got = C.c_size_t(99)
    out = arena.payload(torch.float32)
    assert out.data_ptr() % 16 == 8
    lib, src, samples = cs.eng._lib, C.c_void_p(cs.dev_ragged.data_ptr()), cs.dev_ragged.numel() // cs.r.channels
    if welch(kind) == "csd":
        rc = lib.sgx_csd_batch(cs.eng._ctx, src, samples, first, n, group_of(kind, n), C.c_void_p(out.data_ptr()), C.byref(got))
    else:
        rc = lib.sgx_fbank_cross_batch(bank_of(cs.eng)._h, src, samples, first, n, C.c_void_p(out.data_ptr()), C.byref(got))
    assert rc == _lib.SGX_ERR_INVALID_ARG and got.value == 0, (what, rc, got.value)
    torch.cuda.synchronize()
    assert arena.guards_intact() and torch.equal(arena.words, before), (what, "a refused call wrote")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,kind", SERVED)
def test_output_guards(torch_cuda, name, kind, variant):
    torch = torch_cuda
    cs = case(torch, name)
    rb = row_bytes(cs.eng, kind)
    for first, n in calls_of(cs):
        for second in (False, True):
            prefill = ba.prefill_word(elem_of(kind), second)
            arena = Arena(torch, rows_of(kind, n) * rb, rb, variant == "odd", prefill)
            if (kind == "fbank_cross" or welch(kind) == "csd") and variant == "odd":
                refused_for_alignment(torch, cs, kind, arena, first, n, (name, kind, variant, first, n))
                continue
            run(cs.eng, kind, cs.dev_ragged, first, n, out=arena.payload(dtype_of(torch, kind)))
            what = (name, kind, variant, first, n, "all ones" if second else "+inf")
            check_result(torch, cs, kind, first, n, arena.payload(), what)
            check_arena(arena, prefill, what)


def istft_ranges(cs):
    N, W, H = cs.N, cs.r.W, cs.r.H
    return [(0, N), (1, 1), (W - 1, H + 1), (N - 3, 3), (H, 2 * H + 1)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", INVERSE_ROWS)   # (the rows left out: test_expected_unsupported)
def test_inverse_output_guards(torch_cuda, name, variant):
    torch = torch_cuda
    cs = case(torch, name)
    assert cs.istft == 1
    Cn = cs.r.channels
    for a, n in istft_ranges(cs):
        assert a + n <= cs.N
        for second in (False, True):
            prefill = ba.prefill_word("f32", second)
            arena = Arena(torch, n * Cn * 4, Cn * 4, variant == "odd", prefill)
            cs.eng.istft_batch(cs.spec, first_sample=a, max_samples=n, out=arena.payload(torch.float32))
            what = (name, "istft", variant, a, n, "all ones" if second else "+inf")
            assert torch.equal(arena.payload(), cs.flat["istft"][a * Cn:(a + n) * Cn]), what
            check_arena(arena, prefill, what)


# ---- B: input isolation -------------------------------------------------------------------------------------------------------------
def poisoned_stream(torch, cs, odd, tail, lo, hi):
    """The stream plus `tail` ragged samples as the payload of a NaN arena, every sample outside [lo, hi) NaN as well; the slice handed
    to the library ends with the tail, so n_samples is short of what lies behind it."""
    r = cs.r
    arena = Arena(torch, (cs.N + tail) * r.channels * 4, r.W * r.channels * 4, odd, ba.NAN_WORD, guard=ba.NAN_WORD, mod4=r.align4)
    dev = arena.payload(torch.float32)
    dev[lo * r.channels:hi * r.channels] = cs.dev[lo * r.channels:hi * r.channels]
    return arena, dev


@pytest.mark.parametrize("name,kind", SERVED)
def test_input_isolation(torch_cuda, name, kind):
    torch = torch_cuda
    cs = case(torch, name)
    r = cs.r
    for variant in (VARIANTS if r.channels >= 2 else VARIANTS[:1]):   # (mono: the align4 row is the odd placement)
        for tail in sorted({0, 1, r.H - 1}):
            for first, n in calls_of(cs):
                lo, hi = ba.needed_samples(r, first, n)
                hi = min(hi, cs.N)   # (a partner frame the stream does not hold has no samples)
                arena, dev = poisoned_stream(torch, cs, variant == "odd", tail, lo, hi)
                assert cs.eng.num_frames(dev.numel() // r.channels) == cs.F
                got = run(cs.eng, kind, dev, first, n)
                check_result(torch, cs, kind, first, n, words(torch, got), (name, kind, variant, tail, first, n))


@pytest.mark.parametrize("name", INVERSE_ROWS)
def test_inverse_input_isolation(torch_cuda, name):
    torch = torch_cuda
    cs = case(torch, name)
    assert cs.istft == 1
    r = cs.r
    W, H, Cn = r.W, r.H, r.channels
    per_frame = r.pairs * (W - 1) * 4
    for variant in VARIANTS:
        for a, n in istft_ranges(cs):
            arena = Arena(torch, cs.F * per_frame * 4, per_frame * 4, variant == "odd", ba.NAN_WORD, guard=ba.NAN_WORD)
            spec = arena.payload(torch.float32).view(cs.F, r.pairs, W - 1, 2, 2)
            used = [t for t in range(cs.F) if t * H < a + n and t * H + W > a]   # the frames that cover a requested sample
            assert used
            spec[used[0]:used[-1] + 1] = cs.spec[used[0]:used[-1] + 1]
            if Cn == 1:
                spec[:, :, :, 1, :] = float("nan")   # mono: one channel from the L half (include/sgx.h)
            got = cs.eng.istft_batch(spec, first_sample=a, max_samples=n)
            assert torch.equal(words(torch, got), cs.flat["istft"][a * Cn:(a + n) * Cn]), (name, variant, a, n)


# ---- C: stale state -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_stale_state(torch_cuda, name):
    torch = torch_cuda
    cs = case(torch, name)
    r, F = cs.r, cs.F
    eng = engine(r, gradient="viridis")   # ONE context for the three runs
    hot = to_dev(torch, r, np.full((cs.N, r.channels), 3e38, np.float32))          # the spectra overflow to inf
    nan = to_dev(torch, r, np.full((cs.N, r.channels), np.nan, np.float32))
    kinds = kinds_of(name)
    for stream in (hot, nan):
        for kind in kinds:
            scratch = run(eng, kind, stream, 0, F)
        if cs.istft:
            eng.istft_batch(torch.view_as_real(eng.stft_batch_complex(stream)).contiguous())
    del scratch
    # the workspace between its row layouts (fbank: rows; psd: rows and block partials behind them; fbank_cross: double rows; csd: double
    # rows and double partials), every call of another frame count than its neighbours, on the overflowing stream and then on the real
    # one: a partial row or a resumed block that kept what the last user left shows in the Welch means.  (A mono row has no cross kinds.)
    # No group is carried at these rows' 9, 5, 300 and 70 frames (tests/test_bounds_arena.py: test_welch_cases_of_the_gpu_tests), so the
    # carry row after NaN is left to tests/test_gpu_psd.py's contexts and to part E below.
    assert F >= 5
    layouts = [("fbank", 0, F), ("psd_3", 1, F - 1), ("fbank_cross", 1, F - 2), ("csd_3", 0, F - 3), ("psd_n5", 2, max(F - 5, 2)),
               ("fbank", 2, F - 4)]
    layouts = [c for c in layouts if c[0] in kinds]
    assert all(first + n <= F and n >= 1 for _, first, n in layouts)
    for stream in (hot, cs.dev):
        got = [run(eng, kind, stream, first, n) for kind, first, n in layouts]
    for (kind, first, n), t in zip(layouts, got):
        check_result(torch, cs, kind, first, n, words(torch, t), (name, kind, first, n, "between the workspace's row layouts"))
    del got
    for kind in kinds:
        out = None
        if kind.startswith("peak"):   # (a stale +inf would survive a max: what the buffer held before must not matter either)
            out = torch.full((rows_of(kind, F), eng.pairs, eng.R, 2), float("inf"), dtype=torch.float32, device="cuda")
        got = run(eng, kind, cs.dev, 0, F, out=out)
        check_result(torch, cs, kind, 0, F, words(torch, got), (name, kind, "after an overflowing and an all-NaN stream"))
    if cs.istft:
        got = eng.istft_batch(cs.spec)
        assert torch.equal(words(torch, got), cs.flat["istft"]), (name, "istft after non-finite spectra")
    eng.close()


# ---- D: the pixel-stage entry points ------------------------------------------------------------------------------------------------
PIXEL_CONTEXTS = {
    "w2048_mono": dict(window_samples=2048, hop_samples=256, channels=1),
    "w4096_lr": dict(window_samples=4096, hop_samples=1000, channels=2),
    "w300_lr": dict(window_samples=300, hop_samples=75, channels=2),
    "w2048_rows7": dict(window_samples=2048, hop_samples=256, channels=1, rows=7),
}
PIXEL_RANGES = np.array([[32.0, 64.0], [100.0, 101.0], [440.0, 880.0], [1000.0, 12000.0], [20.0, 23999.0]], np.float32)


def stage_group(cols):
    """the group of the Welch stages under D: columns of 3 frames, and of 33 (two blocks, the last column short) on the long input"""
    return 3 if cols < 100 else 33


def pixel_call(eng, entry, src, out=None):
    if entry == "render_mags":
        return eng.render_mags(src, out=out)
    if entry == "render_bands":
        return eng.render_bands(src, out=out)
    if entry == "fbank_mags":
        return bank_of(eng).apply(src, out=out)
    if entry == "fbank_cross_spec":
        return bank_of(eng).cross_apply(src, out=out)
    if entry == "psd_mags":
        return eng.psd_mags(src, stage_group(src.shape[0]), out=out)
    if entry == "csd_spec":
        return eng.csd_spec(src, stage_group(src.shape[0]), out=out)
    return eng.magnitude_in(src, PIXEL_RANGES, out=out)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("entry", ["render_mags", "render_bands", "magnitude_in", "fbank_mags", "fbank_cross_spec", "psd_mags", "csd_spec"])
@pytest.mark.parametrize("ctx", sorted(PIXEL_CONTEXTS))
def test_pixel_stage(torch_cuda, ctx, entry, variant):
    """(the bank entries: edge_bank's filters on bin 0 and on bin M - 1 of every column would pull the neighbouring column's word, or the
    NaN around the arena's payload, into a sum if a read were one bin off; the Welch entries: rows of frames inside the NaN arena, the
    means of every column against the header's sum order, tests/psd_reference.py -- every context here has one pair, so a column of the
    input is a frame)"""
    torch = torch_cuda
    key = ("pixel", ctx)
    if key not in _cache:
        _cache[key] = SpectrogramEngine(es.SR, device=0, gradient="viridis", **PIXEL_CONTEXTS[ctx])
    eng = _cache[key]
    odd = variant == "odd"
    rng = np.random.default_rng([len(ctx), len(entry)])
    assert eng.pairs == 1
    cross = entry in ("fbank_cross_spec", "csd_spec")
    in_row = {"render_bands": eng.R * 2, "fbank_cross_spec": eng.M * 4, "csd_spec": eng.M * 4}.get(entry, eng.M * 2)   # floats per input column
    out_row = {"magnitude_in": len(PIXEL_RANGES) * 8, "fbank_mags": ba.N_BANK_FILTERS * 8, "fbank_cross_spec": ba.N_BANK_FILTERS * 16,
               "psd_mags": eng.M * 8, "csd_spec": eng.M * 16}.get(entry, eng.R * 4)   # bytes per output column
    for cols in (1, 7, 700):   # 700: the persistent workgroups walk several columns each
        # magnitudes from 1e-6 to 1: the whole of the colour ramp
        host = (10.0 ** rng.uniform(-6.0, 0.0, (cols, in_row // 2, 2))).astype(np.float32)
        if cross:
            host *= rng.choice(np.float32([-1.0, 1.0]), host.shape)
        out_cols = -(-cols // stage_group(cols)) if entry in ("psd_mags", "csd_spec") else cols
        exact_in = torch.from_numpy(host).cuda()
        want = words(torch, pixel_call(eng, entry, exact_in))
        if entry.startswith("fbank"):   # the clean run itself against the definition (tests/fbank_reference.py), on the first and the last column
            bank, ends = fr.edge_bank(eng.M), [0, cols - 1]
            ref = fr.bank_sums(host[ends], bank, 2) if entry == "fbank_mags" else fr.cross_sums(host[ends].reshape(2, eng.M, 2, 2), bank)
            assert np.array_equal(want.view(cols, -1)[ends].cpu().numpy().view(np.uint32).reshape(-1), ref.view(np.uint32).reshape(-1)), (ctx, entry, cols)
        if entry in ("psd_mags", "csd_spec"):   # the clean run itself against the definition, every column
            x = pr.psd_terms(host.reshape(cols, 1, eng.M, 2)) if entry == "psd_mags" else pr.csd_terms(host.reshape(cols, 1, eng.M, 2, 2))
            mean = pr.welch_mean(x, stage_group(cols))
            assert mean.shape[0] == out_cols and np.array_equal(want.cpu().numpy().view(np.uint32), mean.reshape(-1).view(np.uint32)), (ctx, entry, cols)
        src = Arena(torch, cols * in_row * 4, in_row * 4, odd, ba.NAN_WORD, guard=ba.NAN_WORD)
        src.payload(torch.float32)[:] = exact_in.view(-1)
        for second in (False, True):
            prefill = ba.prefill_word(ELEM[entry], second)
            arena = Arena(torch, out_cols * out_row, out_row, odd, prefill)
            out = arena.payload(torch.uint8 if ELEM[entry] == "u8" else torch.float32)
            if cross and odd:   # both buffers must be 16-byte aligned (include/sgx.h): refused, nothing written
                before = arena.words.clone()
                if entry == "csd_spec":
                    got = C.c_size_t(99)
                    rc = eng._lib.sgx_csd_spec(eng._ctx, C.c_void_p(src.payload().data_ptr()), cols, stage_group(cols), C.c_void_p(out.data_ptr()),
                                               C.byref(got))
                    assert got.value == 0, (ctx, entry, variant, cols)
                else:
                    rc = eng._lib.sgx_fbank_cross_spec(bank_of(eng)._h, C.c_void_p(src.payload().data_ptr()), cols, C.c_void_p(out.data_ptr()))
                torch.cuda.synchronize()
                assert rc == _lib.SGX_ERR_INVALID_ARG and torch.equal(arena.words, before), (ctx, entry, variant, cols, rc)
                continue
            pixel_call(eng, entry, src.payload(torch.float32).view(cols, in_row // 2, 2), out=out)
            what = (ctx, entry, variant, cols, "all ones" if second else "+inf")
            assert torch.equal(arena.payload(), want), what
            check_arena(arena, prefill, what)
        assert torch.equal(src.payload(torch.float32).view(-1), exact_in.view(-1)), "the input was written"


# ---- E: chunk seams -----------------------------------------------------------------------------------------------------------------
SEAM = dict(window_samples=8192, hop_samples=16, channels=2, rows=1024)


def seam_engine():
    eng = SpectrogramEngine(es.SR, device=0, gradient="viridis", **SEAM)
    # the two-kernel routes through the workspace; a route or a constant other than bounds_arena restates fails here, nothing adapts
    assert eng.info.stft_kernel == 10 and eng.info.render_path & 1 == 0 and eng.bands_fused == 0 and eng.bands_peak_fused == 0
    assert (eng.W, eng.pairs, eng.R) == (8192, 1, 1024)
    assert eng.info.mags_bytes_per_frame == ba.mags_bytes_per_frame(8192, 1)
    return eng


def test_seams_render_and_bands(torch_cuda):
    torch = torch_cuda
    eng = seam_engine()
    chunk = ba.render_chunk(eng.W, eng.pairs)
    assert chunk == ba.bands_chunk(eng.W, eng.pairs) == 3072   # 3072 frames of magnitudes fill the 192 MiB
    F = 2 * chunk + 37
    assert F > 2 * chunk
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED0909)
    whole = {"render": eng.render_batch(pcm), "bands": eng.bands_batch(pcm)}
    rng = np.random.default_rng(909)
    cuts = sorted(int(c) for c in rng.choice([f for f in range(1, F) if f % chunk], 5, replace=False))
    edges = [0] + cuts + [F]
    for kind in ("render", "bands"):
        assert whole[kind].shape[0] == F
        parts = [run(eng, kind, pcm, a, b - a) for a, b in zip(edges, edges[1:])]
        assert torch.equal(words(torch, torch.cat(parts, 0)), words(torch, whole[kind])), (kind, cuts, "pieces differ from the whole")
    ends = eng.bin_edges()
    ranges = np.stack([ends[:-1], ends[1:]], 1)
    for seam in (chunk, 2 * chunk):   # the six frames around each seam from sgx_stft_batch's own rows
        rows = eng.stft_batch(pcm, seam - 3, 6).reshape(-1, eng.M, 2)
        px = eng.render_mags(rows)
        assert torch.equal(px.view(-1), whole["render"][seam - 3:seam + 3].reshape(-1)), ("render_batch", seam)
        bands = eng.magnitude_in(rows, ranges)
        assert torch.equal(words(torch, bands), words(torch, whole["bands"][seam - 3:seam + 3])), ("bands_batch", seam)


def test_seams_fbank(torch_cuda):
    """sgx_fbank_batch and sgx_fbank_cross_batch across the workspace's chunks: the magnitude rows of 3072 frames fill it, the complex rows
    of 1536 (in_workspace_chunks with two rows per frame), so 2 * 3072 + 37 frames cross two seams of the one loop and four of the other"""
    torch = torch_cuda
    eng = seam_engine()
    chunk, cross_chunk = ba.fbank_chunk(eng.W, eng.pairs), ba.fbank_cross_chunk(eng.W, eng.pairs)
    assert (chunk, cross_chunk) == (3072, 1536)
    F = 2 * chunk + 37
    seams = {"fbank": [s for s in range(chunk, F, chunk)], "fbank_cross": [s for s in range(cross_chunk, F, cross_chunk)]}
    assert len(seams["fbank"]) == 2 and len(seams["fbank_cross"]) == 4
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED090C)
    fb = bank_of(eng)
    assert fb.fused == 0 and fb.cross_fused == 0
    rng = np.random.default_rng(910)
    cuts = sorted(int(c) for c in rng.choice([f for f in range(1, F) if f % cross_chunk], 4, replace=False))   # five pieces
    edges = [0] + cuts + [F]
    for kind in ("fbank", "fbank_cross"):
        whole = run(eng, kind, pcm, 0, F)
        assert whole.shape[0] == F
        parts = [run(eng, kind, pcm, a, b - a) for a, b in zip(edges, edges[1:])]
        assert torch.equal(words(torch, torch.cat(parts, 0)), words(torch, whole)), (kind, cuts, "pieces differ from the whole")
        del parts
        for seam in seams[kind]:   # the six frames around each seam from the engine's own rows
            if kind == "fbank":
                staged = fb.apply(eng.stft_batch(pcm, seam - 3, 6).reshape(-1, eng.M, 2))
            else:
                staged = fb.cross_apply(torch.view_as_real(eng.stft_batch_complex(pcm, seam - 3, 6)).reshape(-1, eng.M, 2, 2))
            assert torch.equal(words(torch, staged), words(torch, whole[seam - 3:seam + 3])), (kind, seam)
    eng.close()


def peak_against_bands(torch, eng, pcm, bands, first, groups):
    n = bands.shape[0] - first
    for g in groups:
        cols = -(-n // g)
        out = torch.full((cols, eng.pairs, eng.R, 2), float("inf"), dtype=torch.float32, device="cuda")
        got = eng.bands_peak_batch(pcm, g, first_frame=first, out=out)
        assert got.shape[0] == cols
        assert same(got, amax_groups(bands[first:], g)), (first, g, "differs from amax over bands_batch")


def test_seams_peak_workspace_route(torch_cuda):
    torch = torch_cuda
    eng = seam_engine()
    F = 6000
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED090A)
    bands = eng.bands_batch(pcm)
    assert bands.shape[0] == F
    for first in (0, 3):
        n = F - first
        chunk = ba.peak_chunk(eng.W, eng.pairs, eng.R, n, n)
        assert chunk == 2688 and n > 2 * chunk
        loop = lambda g: ba.peak_chunks(eng.W, eng.pairs, eng.R, n, g)   # noqa: E731
        # one column over three chunks; two columns, the second chunk trimmed to the end of column 0
        assert [c[2:] for c in loop(n)] == [(0, False), (0, True), (0, True)]
        assert loop(4000)[1] == (chunk, 4000 - chunk, 0, True) and loop(4000)[2][2:] == (1, False)
        assert loop(chunk + 1)[1] == (chunk, 1, 0, True)
        peak_against_bands(torch, eng, pcm, bands, first, [n, n + 5, 4000, chunk + 1, chunk, chunk - 1])


def test_seams_peak_fused_route(torch_cuda):
    torch = torch_cuda
    eng = SpectrogramEngine(es.SR, device=0, window_samples=2048, hop_samples=256, channels=1)
    # (the real-input kernel: two frames per job, as bounds_arena.fused_peak_run restates its split)
    assert eng.bands_peak_fused == 1 and eng.info.render_path & 8 and eng.info.stft_kernel == es.ROUTE["k1r_h256"].kernel
    F = 5000
    pcm = eng.white_noise(eng.W + (F - 1) * eng.H, seed=0x5EED090B)
    bands = eng.bands_batch(pcm)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # the seams of this route are the ends of the persistent workgroups' runs (bounds_arena.fused_peak_run: six frames each on 256 CUs):
    # columns of one run, one frame more and one less, and the long ones the combine pass finishes
    for first in (0, 3):
        n = F - first
        run = ba.fused_peak_run(n, n, n_cu)
        assert 2 <= run and 2 * run < n, "more than two runs, each of more than one frame"
        groups = [n, n + 5, 4000, run + 1, run, run - 1]
        for g in groups:   # as the launcher splits THIS call: no group lengthens the run, so every one but `run` has columns across seams
            assert ba.fused_peak_run(n, min(g, n), n_cu) == run, (g, "the run was aligned to the group")
            assert (run % min(g, n) == 0) == (g == run or g == 1), (g, "no column of this group crosses a run's end")
        peak_against_bands(torch, eng, pcm, bands, first, groups)


# ---- the Welch kinds: the baseline on every sub-range, and the seams of psd_reduce's ranges the model of bounds_arena selects -----------
@pytest.mark.parametrize("name", ROWS)
def test_welch_baseline(torch_cuda, name):
    """On fresh, exact-size tensors: every Welch kind of every (first, n) of calls_of equals the header's sum order over the baseline's own
    rows of that sub-range, the columns counted from its first frame, and the stage over those rows"""
    torch = torch_cuda
    cs = case(torch, name)
    spec = torch.view_as_real(cs.base["complex"]).contiguous()
    for kind in kinds_of(name):
        if not welch(kind):
            continue
        for first, n in calls_of(cs):
            got = words(torch, run(cs.eng, kind, cs.dev, first, n))
            check_result(torch, cs, kind, first, n, got, (name, kind, first, n))
            g = group_of(kind, n)
            staged = cs.eng.psd_mags(cs.base["stft"][first:first + n], g) if welch(kind) == "psd" else cs.eng.csd_spec(spec[first:first + n], g)
            assert torch.equal(words(torch, staged), got), (name, kind, first, n, "the stage over the baseline's rows differs")


def strided_welch(kind, rows, group, stride):
    """the header's sum order on every stride-th bin of rows on the device (as tests/test_gpu_psd.py: strided_reference)"""
    bins = rows[:, :, ::stride].cpu().numpy()
    return pr.welch_mean(pr.psd_terms(bins) if kind == "psd" else pr.csd_terms(bins), group)


def welch_against_rows(torch, eng, kind, pcm, frames, group, stride, what):
    """a batch call against the stage over the engine's own rows (the caller's rows, no row slots in the workspace: another layout of the
    same ranges) on the device, and against the definition on a strided subset of the bins"""
    if kind == "psd":
        rows = eng.stft_batch(pcm)
        got, staged = eng.psd_batch(pcm, group), eng.psd_mags(rows, group)
    else:
        rows = torch.view_as_real(eng.stft_batch_complex(pcm)).contiguous()
        got, staged = eng.csd_batch(pcm, group), eng.csd_spec(rows, group)
    assert rows.shape[0] == frames and got.shape[0] == -(-frames // min(group, frames)), what
    assert torch.equal(words(torch, got), words(torch, staged)), (what, "batch and stage differ")
    want = strided_welch(kind, rows, group, stride)
    assert np.array_equal(got[:, :, ::stride].cpu().numpy().view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)), (what, "not the definition's bits")
    return got


@pytest.mark.parametrize("kind", ["psd", "csd"])
def test_seams_welch_carried_column(torch_cuda, kind):
    """A column with more blocks than a range holds, carried in the context's float64 row, on a family whose rows do not go through kernel
    11's scratch: the route of the table that needs the fewest frames for it (W 8192, 8 channels, hop 300: 737 frames, 353 of complex
    rows) in one column, three more in a second.  The carry row is grown by the first call; the call is then repeated after one on an
    all-NaN stream left NaN sums in it."""
    torch = torch_cuda
    cross = kind == "csd"
    frames, r = ba.welch_carried_route(es.ROUTES, cross)
    total = frames + 3                                     # a second, short column behind the carried one: it starts from +0 again
    plan = ba.welch_ranges(r.W, r.pairs, cross, total, frames, True)
    assert plan.carried and r.kernel != 11
    assert [(x.reads_carry, x.writes_carry) for x in plan.ranges] == [(False, True), (True, False), (False, False)]
    assert plan.ranges[2].frames == (frames, total)
    eng = engine(r)
    assert eng.info.stft_kernel == r.kernel and eng.info.mags_bytes_per_frame == ba.mags_bytes_per_frame(r.W, r.pairs)
    pcm = eng.white_noise(r.W + (total - 1) * r.H, seed=0x5EED090D)
    what = (r.name, kind, total, frames)
    got = welch_against_rows(torch, eng, kind, pcm, total, frames, 64, what)
    nan = torch.full_like(pcm, float("nan"))
    batch = eng.psd_batch if kind == "psd" else eng.csd_batch
    assert bool(torch.isnan(batch(nan, ba.WELCH_MAX)).all())
    assert torch.equal(words(torch, batch(pcm, frames)), words(torch, got)), (what, "after NaN in the carry row")
    eng.close()


def test_seams_welch_odd_frame_of_a_paired_context(torch_cuda):
    """Two frames of one transform (SGX_FLAG_PAIRED_FRAMES, mono W 2048): at group 1 a range holds 12294 // 2 = 6147 frames, so the second
    range's rows launch starts on an odd frame, whose partner lies in the range before"""
    torch = torch_cuda
    r = es.ROUTE["k1_paired_mono"]
    group, frames = ba.welch_odd_seam(r.W, r.pairs)
    plan = ba.welch_ranges(r.W, r.pairs, False, frames, group, True)
    assert len(plan.ranges) == 2 and plan.ranges[1].frames[0] % 2 == 1 and r.paired
    eng = engine(r)
    assert eng.info.stft_kernel == r.kernel and eng.info.mags_bytes_per_frame == ba.mags_bytes_per_frame(r.W, r.pairs)
    pcm = eng.white_noise(r.W + (frames - 1) * r.H, seed=0x5EED090E)
    welch_against_rows(torch, eng, "psd", pcm, frames, group, 64, (r.name, group, frames))
    eng.close()

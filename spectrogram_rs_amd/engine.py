"""SpectrogramEngine -- thin object wrapper over one sgx_ctx (include/sgx.h).

Device buffers are torch tensors (plumbing: allocation, streams); the arithmetic is entirely in
libsgx.so's HIP kernels.  All batch calls take and return tensors on the engine's GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import SgxError, sgx_config, sgx_info


class SpectrogramEngine:
    def __init__(self, sample_rate: float = 48000.0, *, period: float = 0.0, stride: float = 0.0,
                 window_samples: int = 0, hop_samples: int = 0, channels: int = 1, rows: int = 1024,
                 f_min: float = 32.0, f_max: float = 22030.0, min_db: float = -70.0, max_db: float = -10.0,
                 interp: int = _lib.INTERP_CUBIC, lut_index_mode: int = _lib.LUT_FLOOR_N,
                 device: Optional[int] = None, force_generic: bool = False, gradient: Optional[str] = None,
                 fused_render: bool = True, lut_walk: bool = False,
                 mixed_generic: bool = False, complex_mono: bool = False, paired_frames: bool = False,
                 large_transforms: bool = False):
        import torch

        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        cfg = sgx_config()
        self._lib.sgx_config_init(C.byref(cfg))
        cfg.sample_rate = sample_rate
        cfg.period, cfg.stride = period, stride
        if period == 0.0 and window_samples == 0:
            window_samples = 2048
        if stride == 0.0 and hop_samples == 0:
            hop_samples = 256
        cfg.window_samples, cfg.hop_samples = window_samples, hop_samples
        cfg.channels, cfg.rows = channels, rows
        cfg.f_min, cfg.f_max = f_min, f_max
        cfg.min_db, cfg.max_db = min_db, max_db
        cfg.interp, cfg.lut_index_mode = interp, lut_index_mode
        cfg.device = -1 if device is None else int(device)
        cfg.flags = (_lib.FLAG_FORCE_GENERIC if force_generic else 0) | (0 if fused_render else _lib.FLAG_NO_FUSED_RENDER) \
            | (_lib.FLAG_LUT_WALK if lut_walk else 0) | (_lib.FLAG_MIXED_GENERIC if mixed_generic else 0) \
            | (_lib.FLAG_COMPLEX_MONO if complex_mono else 0) | (_lib.FLAG_PAIRED_FRAMES if paired_frames else 0) \
            | (_lib.FLAG_LARGE_TRANSFORM if large_transforms else 0)
        if device is not None and torch.cuda.is_available():
            torch.cuda.set_device(int(device))
        rc = self._lib.sgx_create(C.byref(cfg), C.byref(self._ctx))
        if rc != 0:
            msg = self._lib.sgx_last_error(None).decode()
            self._ctx = C.c_void_p()
            raise SgxError(rc, msg)
        info = self._query()
        self.W, self.P, self.M, self.H = info.window_samples, info.fft_length, info.num_frequencies, info.hop_samples
        self.channels, self.pairs, self.R = info.channels, info.pairs, info.rows
        self.sample_rate = float(sample_rate)
        self.sample_rate_u32 = info.sample_rate_u32
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.use_current_stream()
        if gradient is not None:
            self.set_builtin_gradient(gradient)

    # ---- plumbing --------------------------------------------------------------------------
    def _query(self):
        """sgx_query into self.info (again after a palette change: render_path depends on the colour scheme)"""
        info = sgx_info()
        self._check(self._lib.sgx_query(self._ctx, C.byref(info)))
        self.info = info
        return info

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise SgxError(rc, self._lib.sgx_last_error(self._ctx).decode())
        return rc

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            # rings handed out by live() point into the context: they are destroyed first (include/sgx.h)
            for ref in list(getattr(self, "_rings", ())):
                ring = ref()
                if ring is not None:
                    ring.close()
            self._rings = []
            self._lib.sgx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_current_stream(self):
        """Enqueue on torch's current stream for this device.  Free when the context is on that stream already (sgx_set_stream
        returns at once).  When the stream changes, what the context enqueues from now on is ordered, on the device, behind what it
        has enqueued on the stream it leaves -- its workspace, planes and scratch are shared by both; the host does not wait."""
        import torch

        s = torch.cuda.current_stream(self.device)
        self._check(self._lib.sgx_set_stream(self._ctx, C.c_void_p(s.cuda_stream)))

    def set_stream(self, cuda_stream: int):
        self._check(self._lib.sgx_set_stream(self._ctx, C.c_void_p(cuda_stream)))

    def sync(self):
        self._check(self._lib.sgx_sync(self._ctx))

    def set_cu_limit(self, n: int):
        """Size the persistent launches of later calls for n compute units (0: the device's own count; more than it has is refused).
        Results do not depend on it: an application that shares the GPU with its renderer bounds the engine's footprint this way."""
        self._check(self._lib.sgx_set_cu_limit(self._ctx, C.c_uint32(n)))

    @property
    def cu_limit(self) -> int:
        """the compute-unit count in force"""
        return int(self._lib.sgx_cu_limit(self._ctx))

    def set_run_claim(self, static_sixteenths: int, chunk_jobs: int):
        """Diagnostic: how the rows calls of a mono W 2048 engine deal their frame pairs to the persistent workgroups: (16, 0) one static run
        each, (0, 0) the default rule, else `static_sixteenths` / 16 of them statically and the rest claimed in chunks of `chunk_jobs`.
        Results do not depend on it."""
        self._check(self._lib.sgx_set_run_claim(self._ctx, C.c_uint32(static_sixteenths), C.c_uint32(chunk_jobs)))

    def run_claim(self, n_frames: int):
        """(static_sixteenths, chunk_jobs) a rows call of n_frames frames would run under now; (16, 0): the static split"""
        s, k = C.c_uint32(), C.c_uint32()
        self._check(self._lib.sgx_run_claim(self._ctx, C.c_size_t(n_frames), C.byref(s), C.byref(k)))
        return int(s.value), int(k.value)

    def set_run_weights(self, w=None):
        """Diagnostic: the weights of those calls' static runs, by the workgroup's place on its compute unit: four integers of at least 1
        that sum to 256, (64, 64, 64, 64) for equal runs; None or all zero: the default.  Results do not depend on them."""
        arr = (C.c_uint32 * 4)(*(int(x) for x in w)) if w is not None else None
        self._check(self._lib.sgx_set_run_weights(self._ctx, arr))

    def run_weights(self, n_frames: int):
        """the four weights a float rows call of n_frames frames would run under now"""
        w = (C.c_uint32 * 4)()
        self._check(self._lib.sgx_run_weights(self._ctx, C.c_size_t(n_frames), w))
        return tuple(int(x) for x in w)

    def _dev_f32(self, t):
        import torch

        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), \
            "expected a contiguous float32 CUDA tensor"
        assert t.device == self.device, f"tensor on {t.device}, engine on {self.device}"
        return C.c_void_p(t.data_ptr())

    def _out(self, out, shape, dtype):
        """The caller's output buffer, checked (the kernels write shape-many elements through a raw pointer), or a
        fresh one.  Also re-binds the context to torch's current stream: a batch call is ordered like a torch op -- behind the work
        already on that stream, and, when the engine was last used under another stream, behind the engine's own pending work there
        too (use_current_stream).  The tensors passed in are the caller's to order across streams, as with any torch op."""
        import torch

        self.use_current_stream()
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        need = 1
        for d in shape:
            need *= int(d)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.device == self.device, \
            f"out must be a CUDA tensor on {self.device}"
        assert out.dtype == dtype, f"out must be {dtype}, got {out.dtype}"
        assert out.is_contiguous(), "out must be contiguous"
        assert out.numel() >= need, f"out holds {out.numel()} elements, the call writes {need}"
        return out

    # ---- sizes -----------------------------------------------------------------------------
    def num_frames(self, n_samples: int) -> int:
        return int(self._lib.sgx_num_frames(self._ctx, n_samples))

    # ---- transform -------------------------------------------------------------------------
    def stft_batch(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """pcm: CUDA float32 tensor of n_samples*channels interleaved samples.
        Returns [frames][pairs][M][2] float32 (left, right) magnitudes."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = self._out(out, (n, self.pairs, self.M, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_stft_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                 C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def stft_batch_f16(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """As stft_batch, magnitudes as float16 (l, r) pairs: [frames][pairs][M][2] torch.float16
        (the texel format of the widget's F16F16 ring texture, gpu_spectrogram.rs:218-226)."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = self._out(out, (n, self.pairs, self.M, 2), torch.float16)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_stft_batch_f16(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                     C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def stft_batch_complex(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """The complex spectra behind stft_batch's magnitudes: [frames][pairs][M][2] torch.complex64, (L, R) of bins k = 1..W-1,
        L = DFT(Hann * l) * 2/W and R = DFT(Hann * r) * 2/W, time origin = the frame's first sample (include/sgx.h).  `out`:
        complex64 of that shape, or float32 [frames][pairs][M][2][2] (its view_as_real); the result is a complex64 view of it."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        if out is not None and out.dtype == torch.float32:
            buf = self._out(out, (n, self.pairs, self.M, 2, 2), torch.float32)
        else:
            buf = torch.view_as_real(self._out(out, (n, self.pairs, self.M, 2), torch.complex64))
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_stft_batch_complex(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                         C.c_void_p(buf.data_ptr()), C.byref(got)))
            assert got.value == n
        return torch.view_as_complex(buf.reshape(-1)[:n * self.pairs * self.M * 4].view(n, self.pairs, self.M, 2, 2))

    def istft_batch(self, spec, first_sample: int = 0, max_samples: Optional[int] = None, out=None):
        """The inverse of stft_batch_complex: PCM from complex (L, R) spectra by weighted overlap-add (include/sgx.h states the
        definition).  `spec`: the complex64 [frames][pairs][M][2] that stft_batch_complex returns, or its float32
        [frames][pairs][M][2][2] view.  Returns float32 [n][channels], the samples [first_sample, first_sample + max_samples) that
        exist (n < (frames - 1) * H + W); sample n is stream sample first_frame * H + n of the forward call."""
        import torch

        if spec.dtype == torch.complex64:
            spec = torch.view_as_real(spec)
        per_frame = self.pairs * self.M * 4
        assert spec.dtype == torch.float32 and spec.numel() % per_frame == 0, \
            "expected complex64 [frames][pairs][M][2] or float32 [frames][pairs][M][2][2]"
        n_frames = spec.numel() // per_frame
        total = (n_frames - 1) * self.H + self.W if n_frames else 0
        n = max(total - first_sample, 0)
        if max_samples is not None:
            n = min(n, max_samples)
        buf = self._out(out, (n, self.channels), torch.float32)
        got = C.c_size_t(0)
        self._check(self._lib.sgx_istft_batch(self._ctx, self._dev_f32(spec.contiguous()), n_frames, first_sample, n,
                                              C.c_void_p(buf.data_ptr()), C.byref(got)))
        assert got.value == n
        return buf.reshape(-1)[:n * self.channels].view(n, self.channels)

    def istft_supported(self) -> int:
        """1 when istft_batch serves this context's window, 0 when it does not (the SGX_FLAG_LARGE_TRANSFORM-only lengths)"""
        return self._check(self._lib.sgx_istft_supported(self._ctx))

    def process_one(self, lr: np.ndarray) -> Optional[np.ndarray]:
        """AudioTransform::process on host (l, r) pairs: [n][2] -> [M][2] or None."""
        lr = np.ascontiguousarray(lr, np.float32).reshape(-1, 2)
        out = np.empty((self.M, 2), np.float32)
        rc = self._check(self._lib.sgx_process_one(self._ctx, lr.ctypes.data_as(C.c_void_p), lr.shape[0],
                                                   out.ctypes.data_as(C.c_void_p)))
        return out if rc == 1 else None

    # ---- pixel path ------------------------------------------------------------------------
    def render_batch(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][R][4] uint8 RGBA columns (image-row order: row 0 = top)."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = self._out(out, (n, self.pairs, self.R, 4), torch.uint8)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_render_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                   C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def bands_batch(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][R][2] float32: magnitude_in over the context's rows for every frame, row 0 = the LOWEST
        (the order of bin_edges(); bit-identical to stft_batch followed by magnitude_in over those edges)."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = self._out(out, (n, self.pairs, self.R, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_bands_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                  C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    @property
    def bands_fused(self) -> int:
        """1 when bands_batch runs one fused kernel from PCM to bands in this context, 0 when it runs two"""
        return self._check(self._lib.sgx_bands_fused(self._ctx))

    def bands_peak_batch(self, pcm, group: int, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [ceil(frames / group)][pairs][R][2] float32: the maximum of bands_batch's columns over groups of `group`
        consecutive frames (the last group may be shorter), row 0 = the LOWEST.  group = 1 is bands_batch."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        group = int(group)
        cols = -(-n // group) if group > 0 else 0
        out = self._out(out, (cols, self.pairs, self.R, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_bands_peak_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n,
                                                       min(group, 2 ** 64 - 1), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == cols
        return out

    @property
    def bands_peak_fused(self) -> int:
        """1 when bands_peak_batch runs one kernel from PCM to peak columns (plus a combine pass), 0 on the workspace route"""
        return self._check(self._lib.sgx_bands_peak_fused(self._ctx))

    # ---- Welch-averaged spectra per bin -----------------------------------------------------
    def _welch_batch(self, fn, comps, pcm, group, first_frame, max_frames, out):
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        group = int(group)
        cols = -(-n // group) if group > 0 else 0
        out = self._out(out, (cols, self.pairs, self.M, comps), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(fn(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n, min(group, 2 ** 64 - 1),
                           C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == cols
        return out

    def _welch_rows(self, fn, comps, rows, row_floats, group, out):
        import torch

        assert rows.dtype == torch.float32 and rows.numel() % row_floats == 0, "expected whole float32 rows of this context"
        n = rows.numel() // row_floats
        group = int(group)
        cols = -(-n // group) if group > 0 else 0
        out = self._out(out, (cols, self.pairs, self.M, comps), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(fn(self._ctx, self._dev_f32(rows), n, min(group, 2 ** 64 - 1), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == cols
        return out

    def psd_batch(self, pcm, group: int, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [ceil(frames / group)][pairs][M][2] float32: Welch's estimate per bin, the mean of stft_batch's squared magnitudes
        over groups of `group` consecutive frames (the last group may be shorter).  include/sgx.h states the order of the sum, which
        makes the result a pure function of the rows, and the factors to a power spectrum or a density per Hz.  Mono holds (v, v)."""
        return self._welch_batch(self._lib.sgx_psd_batch, 2, pcm, group, first_frame, max_frames, out)

    def csd_batch(self, pcm, group: int, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [ceil(frames / group)][pairs][M][4] float32: the means over groups of frames of |L|^2, |R|^2, Re L conj R and
        Im L conj R per bin (the products as FilterBank.cross_batch defines them).  A context of at least two channels."""
        return self._welch_batch(self._lib.sgx_csd_batch, 4, pcm, group, first_frame, max_frames, out)

    def psd_mags(self, mags, group: int, out=None):
        """The stage of psd_batch alone: float32 [frames][pairs][M][2] rows, as stft_batch writes them -> [columns][pairs][M][2]"""
        return self._welch_rows(self._lib.sgx_psd_mags, 2, mags, self.pairs * self.M * 2, group, out)

    def csd_spec(self, spec, group: int, out=None):
        """The stage of csd_batch alone: the complex64 [frames][pairs][M][2] that stft_batch_complex returns, or its float32
        [frames][pairs][M][2][2] view -> [columns][pairs][M][4].  Any channel count: mono rows give x0 = x1 = x2 and x3 = +0."""
        import torch

        if spec.dtype == torch.complex64:
            spec = torch.view_as_real(spec)
        return self._welch_rows(self._lib.sgx_csd_spec, 4, spec.contiguous(), self.pairs * self.M * 4, group, out)

    @property
    def psd_fused(self) -> int:
        """1 when psd_batch runs one kernel from PCM to block partials, 0 on the workspace route"""
        return self._check(self._lib.sgx_psd_fused(self._ctx))

    @property
    def csd_fused(self) -> int:
        """1 when csd_batch runs one kernel from PCM to block partials, 0 on the workspace route"""
        return self._check(self._lib.sgx_csd_fused(self._ctx))

    # ---- spectral maxima --------------------------------------------------------------------
    def maxima_batch(self, pcm, k: int, floor: float = 0.0, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][2][k][4] float32: per frame, pair and side the k strongest local maxima of stft_batch's row, strongest
        first (ties: the lower bin), each as (bin, m[bin - 1], m[bin], m[bin + 1]); slots beyond the candidates are zero.  A candidate
        is > its left neighbour, >= its right one and >= floor (include/sgx.h).  Refinement of frequency and level is the caller's."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        k = int(k)
        out = self._out(out, (n, self.pairs, 2, k, 4), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_maxima_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n, C.c_uint32(k),
                                                   C.c_float(floor), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def maxima_mags(self, mags, k: int, floor: float = 0.0, out=None):
        """The stage of maxima_batch alone: float32 [columns][pairs][M][2] rows, as stft_batch writes them -> [columns][pairs][2][k][4]"""
        import torch

        row_floats = self.pairs * self.M * 2
        assert mags.dtype == torch.float32 and mags.numel() % row_floats == 0, "expected whole float32 rows of this context"
        n = mags.numel() // row_floats
        k = int(k)
        out = self._out(out, (n, self.pairs, 2, k, 4), torch.float32)
        if n:
            self._check(self._lib.sgx_maxima_mags(self._ctx, self._dev_f32(mags), n, C.c_uint32(k), C.c_float(floor),
                                                  C.c_void_p(out.data_ptr())))
        return out

    # ---- the cumulative spectrum per frame ------------------------------------------------------
    @staticmethod
    def _shares(p):
        p = [float(x) for x in ([p] if isinstance(p, (int, float)) else p)]
        return (C.c_float * len(p))(*p), len(p)

    def rolloff_batch(self, pcm, power: int, p, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][2][n_p][4] float32: per frame, pair, side and share p[i] in (0, 1] the record (bin, c[bin - 1], c[bin], T):
        the first bin at which the cumulative value c of stft_batch's row (power 1) or of its squares (power 2) reaches rn(p[i] * T), T the
        row's total; (0, 0, 0, T) where T is not > 0.  include/sgx.h fixes the sum order (segments of 32).  Interpolation and Hz are the
        caller's."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        h_p, n_p = self._shares(p)
        out = self._out(out, (n, self.pairs, 2, n_p, 4), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_rolloff_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n, C.c_uint32(int(power)), h_p,
                                                    C.c_uint32(n_p), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def rolloff_mags(self, mags, power: int, p, out=None):
        """The stage of rolloff_batch alone: float32 [columns][pairs][M][2] rows, as stft_batch writes them -> [columns][pairs][2][n_p][4]"""
        import torch

        row_floats = self.pairs * self.M * 2
        assert mags.dtype == torch.float32 and mags.numel() % row_floats == 0, "expected whole float32 rows of this context"
        n = mags.numel() // row_floats
        h_p, n_p = self._shares(p)
        out = self._out(out, (n, self.pairs, 2, n_p, 4), torch.float32)
        if n:
            self._check(self._lib.sgx_rolloff_mags(self._ctx, self._dev_f32(mags), n, C.c_uint32(int(power)), h_p, C.c_uint32(n_p),
                                                   C.c_void_p(out.data_ptr())))
        return out

    # ---- per-bin order statistics over groups of frames ---------------------------------------
    @staticmethod
    def _quantiles(q):
        q = [float(x) for x in ([q] if isinstance(q, (int, float)) else q)]
        return (C.c_double * len(q))(*q), len(q)

    def quantile_batch(self, pcm, group: int, q, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [ceil(frames / group)][n_q][pairs][M][2] float32: per bin and side the order statistics of stft_batch's rows over
        groups of `group` consecutive frames (the last group may be shorter).  q: one value or up to 16 in [0, 1]; the result is the
        word of rank floor(q * (n - 1) + 0.5) among a column's n words, bits unchanged, NaN last (include/sgx.h states the order).
        A column longer than quantile_max_group is refused: quantile_mags over stored rows takes any group."""
        import torch

        n_samples = pcm.numel() // self.channels
        total = self.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        group = int(group)
        h_q, n_q = self._quantiles(q)
        cols = -(-n // group) if group > 0 else 0
        out = self._out(out, (cols, n_q, self.pairs, self.M, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_quantile_batch(self._ctx, self._dev_f32(pcm), n_samples, first_frame, n, min(group, 2 ** 64 - 1),
                                                     h_q, C.c_uint32(n_q), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == cols
        return out

    def quantile_mags(self, mags, group: int, q, out=None):
        """The stage of quantile_batch alone: float32 [frames][pairs][M][2] rows, as stft_batch writes them -> [columns][n_q][pairs][M][2].
        Any group (one column at most), no workspace."""
        import torch

        row_floats = self.pairs * self.M * 2
        assert mags.dtype == torch.float32 and mags.numel() % row_floats == 0, "expected whole float32 rows of this context"
        n = mags.numel() // row_floats
        group = int(group)
        h_q, n_q = self._quantiles(q)
        cols = -(-n // group) if group > 0 else 0
        out = self._out(out, (cols, n_q, self.pairs, self.M, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            self._check(self._lib.sgx_quantile_mags(self._ctx, self._dev_f32(mags), n, min(group, 2 ** 64 - 1), h_q, C.c_uint32(n_q),
                                                    C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == cols
        return out

    @property
    def quantile_max_group(self) -> int:
        """The longest column quantile_batch selects: the frames of rows the 192 MiB workspace holds, at least 1"""
        return int(self._lib.sgx_quantile_max_group(self._ctx))

    # ---- filterbanks ------------------------------------------------------------------------
    def filterbank(self, first, count, weights, power: int = 2) -> "FilterBank":
        """A bank of sparse filters over the M stored bins (include/sgx.h states the definition): filter f weighs the bins
        first[f] .. first[f] + count[f] - 1 with the next count[f] entries of `weights`.  power 1: magnitudes, 2: powers."""
        import weakref

        fb = FilterBank(self, first, count, weights, power)
        if not hasattr(self, "_rings"):
            self._rings = []
        self._rings = [r for r in self._rings if r() is not None] + [weakref.ref(fb)]
        return fb

    def mel_filterbank(self, n_mels: int = 128, f_min: float = 0.0, f_max: Optional[float] = None, scale: str = "htk",
                       norm: Optional[str] = None, power: int = 2) -> "FilterBank":
        """The triangular mel bank of mel_weights() over this engine's bins, as a FilterBank"""
        first, count, weights = mel_weights(self.sample_rate, self.W, n_mels, f_min, f_max, scale, norm)
        return self.filterbank(first, count, weights, power)

    def render_bands(self, bands, out=None):
        """[columns][R][2] float32 band columns (row 0 lowest: bands_batch, bands_peak_batch) -> [columns][R][4] uint8, image order."""
        import torch

        n = bands.numel() // (self.R * 2)
        out = self._out(out, (n, self.R, 4), torch.uint8)
        if n:
            self._check(self._lib.sgx_render_bands(self._ctx, self._dev_f32(bands), n, C.c_void_p(out.data_ptr())))
        return out

    def render_mags(self, mags, out=None):
        """[columns][M][2] float32 magnitudes -> [columns][R][4] uint8."""
        import torch

        n = mags.numel() // (self.M * 2)
        out = self._out(out, (n, self.R, 4), torch.uint8)
        if n:
            self._check(self._lib.sgx_render_mags(self._ctx, self._dev_f32(mags), n, C.c_void_p(out.data_ptr())))
        return out

    def magnitude_in(self, mags, ranges: np.ndarray, out=None):
        """FrequencySample::magnitude_in for every column and every (f0, f1) range:
        mags [columns][M][2] -> [columns][n_ranges][2] float32."""
        import torch

        ranges = np.ascontiguousarray(ranges, np.float32).reshape(-1, 2)
        n = mags.numel() // (self.M * 2)
        out = self._out(out, (n, ranges.shape[0], 2), torch.float32)
        if n and ranges.shape[0]:
            self._check(self._lib.sgx_magnitude_in(self._ctx, self._dev_f32(mags), n, ranges.ctypes.data_as(C.c_void_p),
                                                   ranges.shape[0], C.c_void_p(out.data_ptr())))
        return out

    def spectrum_levels(self, column, levels: np.ndarray) -> np.ndarray:
        """SpectrumAnalyzer::push_frequencies (spectrum_analyzer.rs:46-68) for one column [M][2] on the device;
        `levels` (float64, one per bar) is updated in place and returned."""
        assert levels.dtype == np.float64 and levels.flags.c_contiguous
        assert column.numel() == self.M * 2
        self._check(self._lib.sgx_spectrum_levels(self._ctx, self._dev_f32(column), levels.size,
                                                  levels.ctypes.data_as(C.c_void_p)))
        return levels

    # ---- live capture ----------------------------------------------------------------------
    def live(self, capacity: int = 4096, reference_skip: bool = False) -> "LiveRing":
        """The ring between the audio callback and the GUI tick, consumed side resident on the device."""
        import weakref

        ring = LiveRing(self, capacity, reference_skip)
        if not hasattr(self, "_rings"):
            self._rings = []
        self._rings = [r for r in self._rings if r() is not None] + [weakref.ref(ring)]
        return ring

    def image(self, width: int = 1024) -> "ImageRing":
        """the row-major width x rows RGBA image ring of SimpleSpectrogram (simple_spectrogram.rs:89-94) on the device"""
        return ImageRing(self, width)

    def view(self, viewport_frames: int = 2048) -> "ViewRing":
        """GPUSpectrogram's F16F16 ring texture + fragment program on the device (include/sgx.h: sgx_view)."""
        import weakref

        v = ViewRing(self, viewport_frames)
        if not hasattr(self, "_rings"):
            self._rings = []
        self._rings = [r for r in self._rings if r() is not None] + [weakref.ref(v)]
        return v

    # ---- colour scheme ---------------------------------------------------------------------
    def set_gradient(self, rgb: np.ndarray, stereo: bool = False):
        rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        self._check(self._lib.sgx_set_gradient(self._ctx, rgb.ctypes.data_as(C.c_void_p), rgb.shape[0], int(stereo)))
        self._query()

    def set_gradient_fn(self, fn, stereo: bool = False):
        """Continuous gradient: `fn(t) -> (r, g, b)` stands in for colorous' eval_continuous(t).  It is
        called on the host while the thresholds are built (and by lookup_table), never during a launch."""
        def thunk(t, out, _user):
            r, g, b = fn(t)
            out[0], out[1], out[2] = int(r), int(g), int(b)
        self._gradient_cb = _lib.GRADIENT_FN(thunk)  # keep alive: lookup_table calls it again
        self._check(self._lib.sgx_set_gradient_fn(self._ctx, C.cast(self._gradient_cb, C.c_void_p), None, int(stereo)))
        self._query()

    def set_builtin_scheme(self, name: str, stereo: bool = False):
        """ColorScheme::new_mono / new_stereo with a gradient the library evaluates itself (include/sgx.h)"""
        self._check(self._lib.sgx_set_builtin_scheme(self._ctx, name.encode(), int(stereo)))
        self._query()

    def set_builtin_gradient(self, name: str):
        self._check(self._lib.sgx_set_builtin_gradient(self._ctx, name.encode()))
        self._query()

    def lookup_table(self, resolution: int = 32) -> np.ndarray:
        out = np.empty((resolution, resolution, 4), np.float32)
        self._check(self._lib.sgx_lookup_table(self._ctx, resolution, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- introspection ---------------------------------------------------------------------
    def bin_edges(self) -> np.ndarray:
        out = np.empty(self.R + 1, np.float32)
        self._check(self._lib.sgx_bin_edges(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def row_sample_counts(self) -> np.ndarray:
        out = np.empty(self.R, np.uint32)
        self._check(self._lib.sgx_row_sample_counts(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def window(self) -> np.ndarray:
        out = np.empty(self.W, np.float32)
        self._check(self._lib.sgx_window(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- harness helpers -------------------------------------------------------------------
    def white_noise(self, n_samples: int, first: int = 0, seed: int = 0x5EED0001, channels: Optional[int] = None, out=None):
        import torch

        ch = self.channels if channels is None else channels
        out = self._out(out, (n_samples * ch,), torch.float32)
        self._check(self._lib.sgx_synth_white_noise(self._ctx, C.c_void_p(out.data_ptr()), first, n_samples, ch, seed))
        return out

    def checksum_add(self, t, acc, base_word: int = 0) -> None:
        """Add the checksum of `t` (word indices from base_word) into `acc`, a one-element int64 tensor on this
        device; asynchronous on the current stream (no host round trip)."""
        import torch

        assert acc.is_cuda and acc.device == self.device and acc.dtype == torch.int64 and acc.numel() == 1
        assert t.is_cuda and t.device == self.device and t.is_contiguous()
        self.use_current_stream()
        self._check(self._lib.sgx_checksum_add(self._ctx, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(),
                                               base_word, C.c_void_p(acc.data_ptr())))

    def checksum(self, t, base_word: int = 0) -> int:
        nbytes = t.numel() * t.element_size()
        v = C.c_uint64(0)
        self._check(self._lib.sgx_checksum(self._ctx, C.c_void_p(t.data_ptr()), nbytes, base_word, C.byref(v)))
        return int(v.value)


class LiveRing:
    """sgx_live: ringbuf::HeapRb<(f32, f32)> (audio_input_list_model.rs:30) whose consumer is the hop loop of
    AudioStreamTransform::process (audio_transform.rs:34-42), run on the GPU once per tick."""

    _FORMATS = {"mags": (_lib.LIVE_MAGS, np.float32), "mags_f16": (_lib.LIVE_MAGS_F16, np.float16),
                "rgba": (_lib.LIVE_RGBA, np.uint8), "bands": (_lib.LIVE_BANDS, np.float32)}

    def __init__(self, engine: SpectrogramEngine, capacity: int = 4096, reference_skip: bool = False):
        self.engine = engine
        self.capacity = int(capacity)
        self._lib = engine._lib
        self._h = C.c_void_p()
        engine._check(self._lib.sgx_live_create(engine._ctx, self.capacity,
                                                _lib.LIVE_REFERENCE_SKIP if reference_skip else 0, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sgx_live_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, data, channels: int) -> int:
        """The input callback (audio_input_list_model.rs:63-75): interleaved float32 `data`; returns the pairs
        accepted (overflow is dropped).  Raises SgxError(SGX_ERR_UNSUPPORTED) for more than two channels."""
        data = np.ascontiguousarray(data, np.float32).reshape(-1)
        n = int(self._lib.sgx_live_push(self._h, data.ctypes.data_as(C.c_void_p), data.size, channels))
        if n < 0:
            raise SgxError(n, f"{channels}-channel input not supported!" if n == _lib.SGX_ERR_UNSUPPORTED else "sgx_live_push")
        return n

    def occupied_len(self) -> int:
        return int(self._lib.sgx_live_occupied(self._h))

    def __len__(self) -> int:
        return self.occupied_len()

    def tick(self, what: str = "mags", max_frames: Optional[int] = None) -> np.ndarray:
        """One GUI tick: every complete frame of the ring as a host array
        ("mags": [frames][M][2] f32, "mags_f16": the same in half, "rgba": [frames][R][4] u8,
        "bands": [frames][R][2] f32 -- bands_batch's rows, lowest first)."""
        code, dtype = self._FORMATS[what]
        e = self.engine
        if max_frames is None:
            max_frames = e.num_frames(self.capacity)
        shape = {"rgba": (max_frames, e.R, 4), "bands": (max_frames, e.R, 2)}.get(what, (max_frames, e.M, 2))
        out = np.empty(shape, dtype)
        got = C.c_size_t(0)
        e._check(self._lib.sgx_live_tick(self._h, code, out.ctypes.data_as(C.c_void_p), max_frames, C.byref(got)))
        return out[:got.value]

    def tick_image(self, image: "ImageRing", max_frames: Optional[int] = None) -> int:
        """one GUI tick of SimpleSpectrogram (simple_spectrogram.rs:136-165): every complete frame becomes a pixel column of the image,
        device to device; returns the number of columns written"""
        e = self.engine
        if max_frames is None:
            max_frames = e.num_frames(self.capacity)
        e.use_current_stream()
        got = C.c_size_t(0)
        e._check(self._lib.sgx_live_tick_image(self._h, image._h, max_frames, C.byref(got)))
        return int(got.value)

    def tick_into(self, view: "ViewRing", max_frames: Optional[int] = None) -> int:
        """One GUI tick of the default widget (gpu_spectrogram.rs:255-275): every complete frame of the ring goes, as a half-pair
        row, straight into `view`'s ring texture -- device to device, no host copy.  Returns the number of rows appended."""
        e = self.engine
        if max_frames is None:
            max_frames = e.num_frames(self.capacity)
        got = C.c_size_t(0)
        e._check(self._lib.sgx_live_tick_view(self._h, view._h, max_frames, C.byref(got)))
        return int(got.value)


class FilterBank:
    """sgx_fbank: a bank's tables on the device.  batch(): PCM -> [frames][pairs][n_filters][2] float32 weighted sums of the bin
    magnitudes (power 1) or powers (power 2), (l, r) per filter; apply(): the same from rows already on the device.  Both give the
    same bits (include/sgx.h).  Closed by SpectrogramEngine.close() like the rings."""

    def __init__(self, engine: SpectrogramEngine, first, count, weights, power: int = 2):
        self.engine = engine
        self._lib = engine._lib
        self._h = C.c_void_p()
        first = np.ascontiguousarray(first, np.uint32).reshape(-1)
        count = np.ascontiguousarray(count, np.uint32).reshape(-1)
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        assert first.size == count.size, "first and count hold one entry per filter"
        assert weights.size == int(count.sum(dtype=np.uint64)), "weights holds sum(count) entries"
        if weights.size == 0:
            weights = np.zeros(1, np.float32)   # (a non-null pointer for a bank of empty filters)
        engine.use_current_stream()
        engine._check(self._lib.sgx_fbank_create(engine._ctx, first.size, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                                 weights.ctypes.data_as(C.c_void_p), int(power), C.byref(self._h)))
        self.power = int(power)
        self._n_weights = int(count.sum(dtype=np.uint64))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sgx_fbank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_filters(self) -> int:
        return int(self._lib.sgx_fbank_filters(self._h))

    @property
    def fused(self) -> int:
        """1 when batch() runs one kernel from PCM to sums, 0 on the workspace route (the STFT into a bounded workspace, then the
        stage kernel)"""
        return self.engine._check(self._lib.sgx_fbank_fused(self._h))

    def batch(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][n_filters][2] float32"""
        import torch

        e = self.engine
        n_samples = pcm.numel() // e.channels
        total = e.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = e._out(out, (n, e.pairs, self.n_filters, 2), torch.float32)
        got = C.c_size_t(0)
        if n:
            e._check(self._lib.sgx_fbank_batch(self._h, e._dev_f32(pcm), n_samples, first_frame, n, C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def apply(self, mags, out=None):
        """[columns][M][2] float32 rows (stft_batch's, flattened over pairs) -> [columns][n_filters][2] float32"""
        import torch

        e = self.engine
        n = mags.numel() // (e.M * 2)
        out = e._out(out, (n, self.n_filters, 2), torch.float32)
        if n:
            e._check(self._lib.sgx_fbank_mags(self._h, e._dev_f32(mags), n, C.c_void_p(out.data_ptr())))
        return out

    # ---- the cross sums: |L|^2, |R|^2, Re and Im of L conj R per band (include/sgx.h: sgx_fbank_cross_batch) ----
    @property
    def cross_fused(self) -> int:
        """1 when cross_batch() runs one kernel from PCM to sums, 0 on the workspace route (the complex rows into a bounded
        workspace, then the stage kernel) and on a mono engine"""
        return self.engine._check(self._lib.sgx_fbank_cross_fused(self._h))

    def cross_batch(self, pcm, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][n_filters][4] float32: per band the weighted sums of |L|^2, |R|^2, Re L conj R and Im L conj R.
        The phase is atan2(out3, out2), the correlation out2 / sqrt(out0 out1), the coherence (out2^2 + out3^2) / (out0 out1), the
        mid and side energies out0 + out1 +- 2 out2: all the caller's.  An engine of at least two channels."""
        import torch

        e = self.engine
        n_samples = pcm.numel() // e.channels
        total = e.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = e._out(out, (n, e.pairs, self.n_filters, 4), torch.float32)
        got = C.c_size_t(0)
        if n:
            e._check(self._lib.sgx_fbank_cross_batch(self._h, e._dev_f32(pcm), n_samples, first_frame, n, C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def cross_apply(self, spec, out=None):
        """[columns][M][2][2] float32 complex rows (stft_batch_complex's, flattened over pairs; or its complex64 [columns][M][2]) ->
        [columns][n_filters][4] float32"""
        import torch

        e = self.engine
        if spec.dtype == torch.complex64:
            spec = torch.view_as_real(spec)
        n = spec.numel() // (e.M * 4)
        out = e._out(out, (n, self.n_filters, 4), torch.float32)
        if n:
            e._check(self._lib.sgx_fbank_cross_spec(self._h, e._dev_f32(spec), n, C.c_void_p(out.data_ptr())))
        return out

    # ---- the flux: per band the rise and the fall of every bin against the same bin `lag` frames earlier (include/sgx.h: sgx_flux_batch) ----
    @property
    def flux_max_lag(self) -> int:
        """the largest lag flux_batch() takes: 64 unless a frame's rows are so long that the workspace holds fewer than 65 of them
        (flux_apply() takes 1 .. 64 at any length)"""
        return int(self._lib.sgx_flux_max_lag(self._h))

    def flux_batch(self, pcm, lag: int = 1, first_frame: int = 0, max_frames: Optional[int] = None, out=None):
        """PCM -> [frames][pairs][n_filters][4] float32: per band (rise_l, rise_r, fall_l, fall_r), the weighted sums of the half-wave
        rectified differences of the bank's elements against frame t - lag, rectified per bin before the band sum.  Frames t < lag
        (absolute) are zero.  rise is the spectral flux an onset detector reads; rise - fall telescopes, rise + fall is the L1 distance."""
        import torch

        e = self.engine
        n_samples = pcm.numel() // e.channels
        total = e.num_frames(n_samples)
        n = max(total - first_frame, 0)
        if max_frames is not None:
            n = min(n, max_frames)
        out = e._out(out, (n, e.pairs, self.n_filters, 4), torch.float32)
        got = C.c_size_t(0)
        if n:
            e._check(self._lib.sgx_flux_batch(self._h, e._dev_f32(pcm), n_samples, first_frame, n, int(lag), C.c_void_p(out.data_ptr()), C.byref(got)))
            assert got.value == n
        return out

    def flux_apply(self, mags, lag: int = 1, out=None):
        """[frames][pairs][M][2] float32 rows (stft_batch's) -> [frames][pairs][n_filters][4] float32; frame t is differenced against
        frame t - lag of the same pair, frames t < lag are zero"""
        import torch

        e = self.engine
        n = mags.numel() // (e.pairs * e.M * 2)
        out = e._out(out, (n, e.pairs, self.n_filters, 4), torch.float32)
        if n:
            e._check(self._lib.sgx_flux_mags(self._h, e._dev_f32(mags), n, int(lag), C.c_void_p(out.data_ptr())))
        return out


class ImageRing:
    """sgx_image: the width x rows RGBA Pixbuf of simple_spectrogram.rs:89-94 on the device, written one pixel column per frame at
    `offset` (:140-164) and read back as it lies or as the scrolling picture of :181-209."""

    def __init__(self, engine: SpectrogramEngine, width: int = 1024):
        self.engine = engine
        self.width, self.height = int(width), engine.R
        self._lib = engine._lib
        self._h = C.c_void_p()
        engine._check(self._lib.sgx_image_create(engine._ctx, self.width, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sgx_image_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def offset(self) -> int:
        return int(self._lib.sgx_image_offset(self._h))

    def write_columns(self, rgba) -> int:
        """append [n][rows][4] uint8 pixel columns (a device tensor, e.g. render_batch(...)[:, 0]); returns the new offset"""
        import torch

        e = self.engine
        assert rgba.is_cuda and rgba.device == e.device and rgba.dtype == torch.uint8 and rgba.is_contiguous()
        n = rgba.numel() // (e.R * 4)
        assert rgba.numel() == n * e.R * 4
        e.use_current_stream()
        off = C.c_uint32(0)
        e._check(self._lib.sgx_image_write_columns(self._h, C.c_void_p(rgba.data_ptr()), n, C.byref(off)))
        return int(off.value)

    def read(self, scrolled: bool = False, out=None):
        """[rows][width][4] uint8: the buffer as it lies, or (scrolled) columns [offset, width) followed by [0, offset)"""
        import torch

        e = self.engine
        out = e._out(out, (self.height, self.width, 4), torch.uint8)
        e._check(self._lib.sgx_image_read(self._h, 1 if scrolled else 0, C.c_void_p(out.data_ptr())))
        return out


class ViewRing:
    """sgx_view: the VIEWPORT_FRAMES x (W - 1) F16F16 texture of gpu_spectrogram.rs:218-226 used as a ring (:255-275)
    and the fragment program of :150-186 as a kernel."""

    def __init__(self, engine: SpectrogramEngine, viewport_frames: int = 2048):
        self.engine = engine
        self.rows = int(viewport_frames)
        self._lib = engine._lib
        self._h = C.c_void_p()
        engine._check(self._lib.sgx_view_create(engine._ctx, self.rows, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.sgx_view_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def offset(self) -> int:
        return int(self._lib.sgx_view_offset(self._h))

    def write_rows(self, rows_f16) -> int:
        """append [n][M][2] float16 rows (a device tensor, e.g. stft_batch_f16(...)[:, 0]); returns the new offset"""
        import torch

        e = self.engine
        assert rows_f16.is_cuda and rows_f16.device == e.device and rows_f16.dtype == torch.float16 and rows_f16.is_contiguous()
        n = rows_f16.numel() // (e.M * 2)
        assert rows_f16.numel() == n * e.M * 2
        e.use_current_stream()
        off = C.c_uint32(0)
        e._check(self._lib.sgx_view_write_rows(self._h, C.c_void_p(rows_f16.data_ptr()), n, C.byref(off)))
        return int(off.value)

    def draw(self, width: int, height: int, out=None):
        """the fragment program over a width x height viewport -> [height][width][4] float32, row 0 at the bottom"""
        import torch

        e = self.engine
        out = e._out(out, (height, width, 4), torch.float32)
        e._check(self._lib.sgx_view_draw(self._h, width, height, C.c_void_p(out.data_ptr())))
        return out


def builtin_gradient_eval(name: str, t: float):
    """eval_continuous(t) of a built-in gradient -> (r, g, b)"""
    lib = _lib.load()
    out = (C.c_uint8 * 3)()
    if lib.sgx_builtin_gradient_eval(name.encode(), float(t), out) != 0:
        raise KeyError(name)
    return tuple(int(x) for x in out)


def builtin_gradient(name: str) -> np.ndarray:
    lib = _lib.load()
    out = np.empty((256, 3), np.uint8)
    if lib.sgx_builtin_gradient(name.encode(), out.ctypes.data_as(C.c_void_p)) != 0:
        raise KeyError(name)
    return out


_MEL_SCALES = {"htk": _lib.MEL_HTK, "slaney": _lib.MEL_SLANEY}
_MEL_NORMS = {None: _lib.MEL_NORM_NONE, "none": _lib.MEL_NORM_NONE, "slaney": _lib.MEL_NORM_SLANEY}


def mel_weights(sample_rate: float, window_samples: int, n_mels: int = 128, f_min: float = 0.0, f_max: Optional[float] = None,
                scale: str = "htk", norm: Optional[str] = None):
    """sgx_mel_weights: the triangular mel bank over the true bin frequencies k * sample_rate / (2 W), k = 1 .. W - 1, as
    (first [n_mels] uint32, count [n_mels] uint32, weights [sum(count)] float32).  Host only: no device is touched.
    f_max None: sample_rate / 2.  scale "htk" | "slaney"; norm None | "slaney"."""
    lib = _lib.load()
    if f_max is None:
        f_max = sample_rate / 2.0
    args = (C.c_double(sample_rate), int(window_samples), int(n_mels), C.c_double(f_min), C.c_double(f_max), _MEL_SCALES[scale], _MEL_NORMS[norm])
    n = C.c_size_t(0)
    rc = lib.sgx_mel_weights(*args, None, None, None, C.byref(n))
    if rc != 0:
        raise SgxError(rc, "sgx_mel_weights: invalid argument")
    first, count = np.zeros(n_mels, np.uint32), np.zeros(n_mels, np.uint32)
    weights = np.zeros(max(n.value, 1), np.float32)
    rc = lib.sgx_mel_weights(*args, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc != 0:
        raise SgxError(rc, "sgx_mel_weights: invalid argument")
    return first, count, weights[:n.value]

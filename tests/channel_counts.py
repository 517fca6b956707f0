"""Every transform family at 6, 12 and 64 channels and at the cap of 32 768 (a plain helper of tests/test_channel_counts.py and
tests/test_gpu_channel_counts.py: no GPU, no torch at import).

sgx_create accepts 1, 2 or any even channel count up to 32 768; the route table of tests/edge_signals.py stops at 8 channels: 1, 2 and 4
pairs, a multiple of 4 channels wherever there is more than one pair, every division of the launchers exact.  TABLE repeats the shapes that
table already proves at
   6 channels:  3 pairs, C % 4 != 0 (the 8-byte de-interleave is the whole path, no division of the 16384-point launcher is exact),
  12 channels:  6 pairs, C % 4 == 0 (once more from a stream at 8 modulo 16 bytes: the narrow de-interleave, the same bytes),
  64 channels: 32 pairs,
and CAP_ROWS run 32 768 channels, the largest count the 32-bit lane and row offsets of the kernels allow (the two bounds are restated in
tests/test_channel_counts.py).  Every case pins info.stft_kernel and the render_path bits, as edge_signals.Route does.

The streams are seeded white noise per channel (the floors of conftest.py were measured on white noise), pair p at the gain 2^-(p mod 4):
neighbouring pairs differ in level as well as in content, and a power of two changes no rounding.  The cap rows would need 16 384 float64
truths; their streams are LABELLED instead: 256 distinct base pairs of noise, pair p carries base label(p) = lowbias32(p) mod 256.  The
truth is then 256 transforms and every one of the 16 384 rows is still held to its own.  labelling_shares() states what the labelling
must separate: the index errors that offset arithmetic can make (a pair p read as p + d for small d, powers of two and their
neighbours)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import edge_signals as es
import oracle
from conftest import FLOOR_K16, FLOOR_WIDE, REL_TOL, chirpz_bound

R1, R4, R8 = es.R1, es.R4, es.R8
COUNTS = (6, 12, 64)
CAP = 32768                    # sgx_create: at most 32768 channels
N_LABELS = 256
AMPLITUDE = np.float32(0.25)   # tests/test_gpu_complex.py: white noise at a quarter of full scale
MAX_HOST_BYTES = int(2.5 * 2 ** 30)

# family: (W, H, flags, kernel, bits_set, bits_clear, bands_fused, frames, frames at the cap or None)
# bands_fused: the 4096-point kernels and the compile-time mixed-radix plan run sgx_bands_batch in one kernel (tests/test_gpu_bands.py)
SHAPES = {
    "k1_h256": (2048, 256, (), 2, 0, R8, 1, 9, 1),
    "k1_h58": (2048, 58, (), 2, 0, R8, 1, 9, None),
    "k16_h512": (8192, 512, (), 10, 0, 0, 0, 9, 1),
    "k16_h300": (8192, 300, (), 10, 0, 0, 0, 9, None),
    "mixed_w2400": (2400, 93, (), 9, R4, R8, 1, 9, None),      # more than two channels at W 2400: the mixed-radix kernel (kernel 9 by W)
    "mixed_w735_runtime": (735, 200, (), 6, 0, R4 | R8, 0, 9, 2),
    "chirpz_w1102": (1102, 275, (), 4, R4, R8, 0, 9, None),
    "bluestein_w23": (23, 5, (), 4, 0, R4 | R8, 0, 9, 2),
    "generic_w64": (64, 16, (), 0, 0, R4 | R8, 0, 9, 2),
    "large_w10290": (10290, 5148, ("large_transforms",), 11, 0, 0, 0, 7, None),
    "large_w6001_chirp": (6001, 3003, ("large_transforms",), 11, 0, 0, 0, 7, None),
}
LARGE_BOUND = 1.0              # tests/test_gpu_large.py: LARGE_BOUND["default"] (asserted equal in tests/test_gpu_channel_counts.py)


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    route: es.Route
    frames: int
    cap: bool = False
    # the cap rows of the 4096- and 16384-point kernels run rows, half rows, pixels, bands and peak columns only: their complex rows
    # (2 GiB at W 8192) and filterbank sums are left to the 6-, 12- and 64-channel rows of the same families
    complex_and_banks: bool = True

    @property
    def W(self):
        return self.route.W

    @property
    def H(self):
        return self.route.H

    @property
    def channels(self):
        return self.route.channels

    @property
    def pairs(self):
        return self.route.pairs

    @property
    def samples(self):
        return (self.frames - 1) * self.H + self.W

    @property
    def bound(self) -> float:
        """multiples of the floor the rows are held to: the project's own white-noise bounds"""
        k = self.route.kernel
        return chirpz_bound(self.W) if k == 4 else LARGE_BOUND if k == 11 else 1.0

    @property
    def bands_fused(self) -> int:
        return self.route.bands_fused

    @property
    def bank_fused(self) -> int:
        """sgx_bands_peak_fused, sgx_fbank_fused and sgx_fbank_cross_fused: the 4096-point kernels alone (bounds_arena.fbank_fused)"""
        return 1 if self.route.kernel == 2 else 0

    @property
    def inverse(self) -> bool:
        """sgx_istft_supported: every length but those only the multi-pass transform serves"""
        return self.route.kernel != 11 and self.complex_and_banks

    def engine_kwargs(self, **extra) -> dict:
        kw = self.route.engine_kwargs()
        if self.cap:
            kw["rows"] = 16     # pixel and band columns of 16 rows: 16 384 pairs of them stay small
        kw.update(extra)
        return kw

    def host_bytes(self) -> int:
        """an upper bound of what the host holds of a case at one time, with S the stream and R one float32 output of rows.  The 6-, 12- and
        64-channel rows: S, the rows, their float64 truth (2 R) and the complex rows (2 R).  The cap rows compare on the device and hold S
        alone.  Where the inverse runs: also the complex rows (2 R), its output (S), the float64 reference and the definition's
        accumulator (2 S each)."""
        S, R = self.samples * self.channels * 4, self.frames * self.pairs * (self.W - 1) * 8
        held = S if self.cap else S + 5 * R
        return held + (2 * R + 5 * S if self.inverse else 0)


def _case(family, channels, cap=False):
    W, H, flags, kernel, bits_set, bits_clear, bands_fused, frames, cap_frames = SHAPES[family]
    name = f"{family}_cap" if cap else f"{family}_ch{channels}"
    route = es.Route(name, W, H, channels, tuple(flags), kernel=kernel, bits_set=bits_set, bits_clear=bits_clear,
                     floor=FLOOR_K16 if W == 8192 else FLOOR_WIDE, bands_fused=bands_fused)
    return Case(name, family, route, cap_frames if cap else frames, cap, not (cap and kernel in (2, 10)))


TABLE = [_case(f, c) for f in SHAPES for c in COUNTS]
CAP_ROWS = [_case(f, CAP, cap=True) for f in ("generic_w64", "bluestein_w23", "mixed_w735_runtime", "k1_h256", "k16_h512")]
ALL = TABLE + CAP_ROWS
CASE = {c.name: c for c in ALL}
assert len(CASE) == len(ALL)
# the rows whose compute-unit sweep moves `pairs <= n_cu`, `n_cu / pairs` and the inverse's max(1, ...) across their ends (3 pairs)
CU_ROWS = ["k1_h256_ch6", "k1_h58_ch6", "k16_h512_ch6", "k16_h300_ch6", "mixed_w2400_ch6"]


def cu_limits(pairs: int) -> tuple:
    return (1, pairs - 1, pairs, pairs + 1, 2 * pairs + 1)


# ---- the labelling of the cap rows -------------------------------------------------------------------------------------------------------
def lowbias32(x):
    """the integer hash of the library's noise generator (oracle/spectro_oracle.c: orc_lowbias32), on uint32 arrays"""
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


@functools.lru_cache(maxsize=None)
def labels(pairs: int = CAP // 2) -> np.ndarray:
    lab = (lowbias32(np.arange(pairs, dtype=np.uint32)) % np.uint32(N_LABELS)).astype(np.int64)
    lab.setflags(write=False)
    return lab


def label_distances(pairs: int = CAP // 2) -> list:
    """the pair distances an index error of offset arithmetic can have: 1 .. 8, 2^k, 2^k - 1 and 3 2^k below `pairs`"""
    d = set(range(1, 9))
    k = 0
    while (1 << k) < pairs:
        d.update((1 << k, (1 << k) - 1, 3 << k))
        k += 1
    return sorted(x for x in d if 0 < x < pairs)


def labelling_shares(pairs: int = CAP // 2) -> dict:
    """d -> the share of pairs p with label(p) == label(p + d): a row read from pair p + d passes unnoticed on that share only"""
    lab = labels(pairs)
    return {d: float((lab[:-d] == lab[d:]).mean()) for d in label_distances(pairs)}


# ---- the streams -------------------------------------------------------------------------------------------------------------------------
def _seed(case: Case) -> int:
    return 0xC4A0 + 97 * list(SHAPES).index(case.family) + case.channels


def gain(pair: int) -> np.float32:
    return np.float32(2.0 ** -(pair % 4))


@functools.lru_cache(maxsize=4)
def base_pairs(case: Case) -> np.ndarray:
    """[N_LABELS][samples][2]: the distinct (l, r) base pairs of a cap row"""
    n = case.samples
    x = np.stack([oracle.white_noise(n, seed=_seed(case) + c) for c in range(2 * N_LABELS)], 1) * AMPLITUDE
    x = np.ascontiguousarray(x.reshape(n, N_LABELS, 2).transpose(1, 0, 2))
    x.setflags(write=False)
    return x


def build_stream(case: Case) -> np.ndarray:
    """[samples][channels] float32.  The 6-, 12- and 64-channel rows: channel c is oracle.white_noise(seed + c) at a quarter of full scale
    times its pair's gain.  The cap rows: pair p carries base_pairs(case)[label(p)]."""
    n, C = case.samples, case.channels
    if case.cap:
        base = base_pairs(case)                                        # [labels][n][2]
        return np.ascontiguousarray(base.transpose(1, 0, 2)[:, labels(case.pairs), :]).reshape(n, C)
    pcm = np.empty((n, C), np.float32)
    for c in range(C):
        pcm[:, c] = oracle.white_noise(n, seed=_seed(case) + c) * (AMPLITUDE * gain(c // 2))
    return pcm


def identical_stream(case: Case, frames: int | None = None) -> np.ndarray:
    """[samples][channels]: the same (l, r) in every pair"""
    n = ((case.frames if frames is None else frames) - 1) * case.H + case.W
    lr = np.stack([oracle.white_noise(n, seed=_seed(case) + 0x1D00 + c) for c in range(2)], 1) * AMPLITUDE
    return np.ascontiguousarray(np.tile(lr, (1, case.pairs)))


def frame_of(case: Case, pcm: np.ndarray, t: int) -> np.ndarray:
    return pcm[t * case.H:t * case.H + case.W]


def truth_rows(case: Case, pcm: np.ndarray) -> np.ndarray:
    """[frames][pairs][W - 1][2] float64: es.truth_frame of every frame and pair of a 6-, 12- or 64-channel stream"""
    assert not case.cap
    return np.stack([np.stack([es.truth_frame(es.frame_lr(frame_of(case, pcm, t), p), case.W) for p in range(case.pairs)])
                     for t in range(case.frames)])


def device_ratio(torch, x, ref, floor: float):
    """conftest.mags_error per row in torch float64, on whatever device the tensors lie: x, ref [..., M, 2] -> [...]"""
    x, ref = x.to(torch.float64), ref.to(torch.float64)
    peak = ref.abs().amax(dim=(-1, -2), keepdim=True)
    allow = (REL_TOL * torch.maximum(ref.abs(), floor * peak)).clamp_min(1e-30)
    return ((x - ref).abs() / allow).amax(dim=(-1, -2))


def device_complex_ratio(torch, x, ref, floor: float):
    """test_gpu_complex.complex_error per row (the peak the row's own) in torch complex128: x, ref [..., M, 2] complex -> [...]"""
    x, ref = x.to(torch.complex128), ref.to(torch.complex128)
    mod = ref.abs()
    peak = mod.amax(dim=(-1, -2), keepdim=True)
    allow = (REL_TOL * torch.maximum(mod, floor * peak)).clamp_min(1e-30)
    return ((x - ref).abs() / allow).amax(dim=(-1, -2))


def inverse_ratio(torch, got, ref, env, W: int, H: int, win: np.ndarray, tol: float, device="cpu") -> float:
    """test_gpu_istft.check_definition, formula for formula, with the local peak (max |ref| over [n - W, n + W] and the channel pair) as a
    max-pool on `device` instead of a sliding window view on the host: 64 channels at W 8192 are 10^10 comparisons.  got [N][ch] float32,
    ref [N][ch] float64, env [N] float64.  Returns the worst ratio of |got - ref| to its bound; asserts what check_definition asserts."""
    from test_gpu_istft import interior_min_env
    e_int = interior_min_env(W, H, win) if H <= W // 2 else 1e-3 * env.max()
    assert np.isfinite(got).all()
    zero = env == 0
    assert (got[zero] == 0.0).all(), "the output must be exactly 0 where the envelope is 0"
    ok = env >= 1e-3 * e_int
    if not ok.any():
        return 0.0
    m = torch.from_numpy(np.abs(ref)).to(device)
    if m.shape[1] >= 2:
        m = m.reshape(m.shape[0], -1, 2).amax(dim=2).repeat_interleave(2, dim=1)
    peak = torch.nn.functional.max_pool1d(m.T.contiguous()[None], kernel_size=2 * W + 1, stride=1, padding=W)[0].T   # (|ref| >= 0: the padding never wins)
    scale = np.maximum(1.0, e_int / np.where(env > 0, env, 1.0))
    bound = tol * peak.clamp_min(1e-30) * torch.from_numpy(scale).to(device)[:, None]
    ratio = (torch.from_numpy(np.ascontiguousarray(got)).to(device).to(torch.float64) - torch.from_numpy(ref).to(device)).abs() / bound
    return float(ratio[torch.from_numpy(ok).to(device)].max())


def truth_labels(case: Case) -> np.ndarray:
    """[frames][N_LABELS][W - 1][2] float64: es.truth_frame of every frame of every base pair of a cap row; row (t, p) of the engine is
    held to [t][label(p)]"""
    base = base_pairs(case)
    return np.stack([np.stack([es.truth_frame(base[k, t * case.H:t * case.H + case.W], case.W) for k in range(N_LABELS)])
                     for t in range(case.frames)])

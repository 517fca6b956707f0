"""The case table of tests/test_gpu_stream_routes.py: which entry points run on which route when the context's stream is held back (a
plain helper: no GPU, no torch at import time; tests/test_stream_cases.py checks it).

Every other GPU file runs on torch's default stream, the legacy NULL stream, where a helper pass launched on stream 0 is ordered exactly
like one launched on the context's stream.  The sweep runs every row of edge_signals.ROUTES on a non-default stream that a sleep kernel
holds back: a kernel, copy or memset on another stream runs before its input exists.  The table names, per row, the entry points the row's
route serves, in the order the test calls them, and -- from what the context reports about its routes -- the helper passes each call takes
besides its main kernel (the passes a launcher could misplace one by one)."""
from __future__ import annotations

from dataclasses import dataclass

import bounds_arena as ba
import edge_signals as es

PEAK_GROUP = 3
# the order of the calls: the batch entry points, then the calls that consume what those just made
BATCH = ("stft", "f16", "complex", "render", "bands", "peak_3", "fbank", "fbank_cross", "psd_3", "csd_3")
STAGE = ("render_mags", "magnitude_in", "render_bands", "checksum_add", "fbank_mags", "fbank_cross_spec", "psd_mags", "csd_spec")
ENTRIES = BATCH + ("istft",) + STAGE
SYMBOL = {"stft": "sgx_stft_batch", "f16": "sgx_stft_batch_f16", "complex": "sgx_stft_batch_complex", "render": "sgx_render_batch",
          "bands": "sgx_bands_batch", "peak_3": "sgx_bands_peak_batch", "istft": "sgx_istft_batch", "render_mags": "sgx_render_mags",
          "magnitude_in": "sgx_magnitude_in", "render_bands": "sgx_render_bands", "checksum_add": "sgx_checksum_add",
          "fbank": "sgx_fbank_batch", "fbank_cross": "sgx_fbank_cross_batch", "fbank_mags": "sgx_fbank_mags", "fbank_cross_spec": "sgx_fbank_cross_spec",
          "psd_3": "sgx_psd_batch", "csd_3": "sgx_csd_batch", "psd_mags": "sgx_psd_mags", "csd_spec": "sgx_csd_spec"}
# what a call reads that another call of the same run wrote: a wrong input makes a wrong output whatever the call itself does
READS = {"istft": "complex", "render_mags": "stft", "magnitude_in": "stft", "render_bands": "bands", "checksum_add": "stft",
         "fbank_mags": "stft", "fbank_cross_spec": "complex", "psd_mags": "stft", "csd_spec": "complex"}
# entry points that wait on the host in their steady state, with the reason (include/sgx.h's conventions name them): none
HOST_WAITS: dict = {}

FRAMES = 23            # 8 peak columns at group 3, the last of two frames; more frames than one run of a persistent workgroup
FRAMES_LONG = 5        # W >= 65536 (a frame of 0.5 .. 8 MiB of samples): two columns, the last of two frames
LONG_W = 65536
SEED_A, SEED_B = 0x5EED0A00, 0x5EED0B00


def frames_of(r: es.Route) -> int:
    return FRAMES_LONG if r.W >= LONG_W else FRAMES


def istft_served(r: es.Route) -> bool:
    """sgx_istft_supported: every length an in-LDS kernel serves (stft_istft.hip: istft_route)"""
    return r.kernel != 11


def peak_fused(r: es.Route) -> int:
    """sgx_bands_peak_fused at the default 1024 rows: the 4096-point kernels, unless a mono stream's frames are paired"""
    return int(r.kernel == 2 and not r.paired)


def fbank_cross_served(r: es.Route) -> bool:
    """sgx_fbank_cross_batch: a context with an (l, r) pair (a mono context answers SGX_ERR_UNSUPPORTED); the stage serves every context"""
    return r.channels >= 2


def csd_served(r: es.Route) -> bool:
    """sgx_csd_batch: a context with an (l, r) pair, as sgx_fbank_cross_batch; sgx_csd_spec serves every context"""
    return r.channels >= 2


def psd_fused(r: es.Route) -> int:
    """sgx_psd_fused and sgx_csd_fused: no context runs a fused Welch mode in this build"""
    return 0


def entries_served(r: es.Route) -> tuple:
    return tuple(e for e in ENTRIES if (e != "istft" or istft_served(r)) and (e != "fbank_cross" or fbank_cross_served(r))
                 and (e != "csd_3" or csd_served(r)))


@dataclass(frozen=True)
class Case:
    row: str
    entry: str

    @property
    def route(self) -> es.Route:
        return es.ROUTE[self.row]


CASES = [Case(r.name, e) for r in es.ROUTES for e in entries_served(r)]


def by_row() -> dict:
    out: dict = {}
    for c in CASES:
        out.setdefault(c.row, []).append(c.entry)
    return out


# ---- the helper passes -------------------------------------------------------------------------------------------------------------------
HELPERS = ("deinterleave", "k16_plane", "to_half", "workspace", "workspace_render", "workspace_magnitude_in", "workspace_peak",
           "peak_combine", "ladder", "large_passes", "inverse", "workspace_fbank", "workspace_fbank_cross", "workspace_psd_blocks",
           "workspace_psd_combine")


def family(r: es.Route) -> str:
    """the transform family of the row's rows (sgx_api.hip: stft_route), from what ROUTES pins"""
    if r.kernel == 9:   # the 4800-point kernel: one or two channels, not real-input mode; else the mixed-radix kernels
        return "w4800" if r.channels <= 2 and not r.bits_set & es.R8 else "mixed"
    if r.kernel == 4:
        return "chirpz" if r.bits_set & es.R4 else "bluestein"
    return {0: "generic", 2: "wg4096", 6: "mixed", 10: "w16384", 11: "large"}[r.kernel]


def rows_helpers(r: es.Route) -> set:
    """what a launch of the row's rows runs besides one kernel"""
    out = set()
    fam = family(r)
    if fam == "wg4096" and r.channels > 2:
        out.add("deinterleave")
    if fam == "w16384" and r.channels == 1 and not r.paired:
        out.add("k16_plane")
    if fam in ("chirpz", "bluestein"):
        out.add("ladder")
    if fam == "large":
        out.add("large_passes")
    return out


def helpers(r: es.Route, entry: str, render_fused: bool, bands_fused: bool) -> set:
    """the helper passes of one call, given the two routes the context reports (render_path bit 0, sgx_bands_fused)"""
    fam = family(r)
    rows = rows_helpers(r)
    if entry in ("stft", "complex"):
        return rows
    if entry == "f16":
        return rows if fam in ("wg4096", "w4800", "mixed") else rows | {"workspace", "to_half"}
    if entry == "render":
        # (the fused pixels of a W 2400 context are the mixed-radix kernel's: one kernel whatever the rows' family)
        return (rows if fam == "wg4096" else set()) if render_fused else rows | {"workspace", "workspace_render"}
    if entry == "bands":
        return rows if bands_fused else rows | {"workspace", "workspace_magnitude_in"}
    if entry == "peak_3":
        if peak_fused(r):
            return rows | {"peak_combine"}
        return helpers(r, "bands", render_fused, bands_fused) | {"workspace", "workspace_peak"}
    if entry == "istft":
        return {"inverse"}
    if entry in ("fbank", "fbank_cross"):
        # the bank of the sweep lies within the fused size (bounds_arena.fbank_fused): one kernel behind the rows' own helpers -- the
        # de-interleave pass of 4 and 8 channels -- or the rows (magnitudes, complex) into the workspace and the stage kernel over them
        if ba.fbank_fused(r, cross=entry == "fbank_cross"):
            return rows
        return rows | {"workspace", "workspace_" + entry}
    if entry in ("psd_3", "csd_3"):
        # the rows (magnitudes, complex) into the front of the workspace behind the rows' own helpers, then the two kernels of sgx_psd.hip:
        # block partials behind the rows, the float64 chain over them
        assert not psd_fused(r)
        return rows | {"workspace", "workspace_psd_blocks", "workspace_psd_combine"}
    if entry in ("psd_mags", "csd_spec"):
        return {"workspace_psd_blocks", "workspace_psd_combine"}     # the same two kernels over the caller's rows
    return set()


# ---- the stand-alone objects ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ViewCase:
    name: str
    W: int
    H: int
    channels: int
    viewport: int      # rows of the ring: fewer than the frames written, so that the copy wraps
    frames: int        # rows per write; two writes bring the ring back to the same offset (a view is warmed: its first draw uploads the palette)
    width: int
    height: int


VIEW_CASES = [ViewCase("view_k1r", 2048, 256, 1, 16, 24, 300, 37), ViewCase("view_w1024_lr", 1024, 100, 2, 10, 25, 257, 64)]


@dataclass(frozen=True)
class ImageCase:
    name: str
    W: int
    H: int
    channels: int
    width: int         # fewer columns than the frames written: the ring laps itself and the scrolled read composes two parts


IMAGE_CASES = [ImageCase("image_w1024_lr", 1024, 100, 2, 19)]


@dataclass(frozen=True)
class PixelCase:
    name: str
    body: str          # far_offsets.pixel_body: the kernel body the context must take
    entry: str         # render_mags, magnitude_in
    W: int
    R: int
    large: bool = False
    n_lut: int = 256
    n_ranges: int = 64
    cols: int = 7


# one context per kernel body of the stand-alone pixel stage (far_offsets.PIXEL_CASES at a handful of columns)
PIXEL_CASES = [
    PixelCase("two_pass_w64", "render_two_pass_kernel", "render_mags", 64, 126),
    PixelCase("staged_w10290", "render_kernel<true>", "render_mags", 10290, 20578, large=True),
    PixelCase("unstaged_w20481", "render_kernel<false>", "render_mags", 20481, 40960, large=True),
    PixelCase("far_tables_w64", "render_far_tables_kernel<true>", "render_mags", 64, 126, n_lut=40706),
    PixelCase("magnitude_in_w64", "magnitude_in_kernel<true>", "magnitude_in", 64, 126),
    PixelCase("magnitude_in_w20481", "magnitude_in_kernel<false>", "magnitude_in", 20481, 1024, large=True, n_ranges=20480),
]

@dataclass(frozen=True)
class WelchCase:
    name: str
    W: int
    H: int
    channels: int
    frames: int
    group: int
    cross: bool


# a context where bounds_arena.welch_ranges says the call is both carried (the float64 sums of its one column wait in the context's carry
# row, grown on the stream by the call under test) and pieced (a block's rows a few frames at a time, the later pieces resumed):
# tests/test_gpu_psd.py's W 32768 context of 64 channels
WELCH_CASES = [WelchCase("psd_w32768_ch64", 32768, 8192, 64, 36, ba.WELCH_MAX, False),
               WelchCase("csd_w32768_ch64", 32768, 8192, 64, 36, ba.WELCH_MAX, True)]


# rebinding a busy context: (name, engine keywords, the wrapper's method)
REBIND_CASES = [
    ("seam_bands", dict(window_samples=8192, hop_samples=16, channels=2), "bands_batch"),
    ("seam_render", dict(window_samples=8192, hop_samples=16, channels=2), "render_batch"),
    ("k16_mono_bands", dict(window_samples=8192, hop_samples=512, channels=1), "bands_batch"),
    # a bank created while the context is bound to the first stream (sgx_fbank_create's uploads go there), used from the second: the method
    # is the FilterBank's
    ("seam_fbank", dict(window_samples=8192, hop_samples=16, channels=2), "fbank_batch"),
]

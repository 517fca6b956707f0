"""The pixel stage at every end of its run-time plans, against the oracle, all through the C ABI (tests/pixel_plans.py: the sweep, from
the launchers' rules as the tests restate them; tests/test_pixel_plans.py checks the sweep on the CPU).

launch_render picks one of nine two-pass shapes times three colour modes or a per-column kernel from the window, the row table, the LDS
sizes, the palette and two host-side proofs; wg4096_init and the mixed-radix *_column_fits decide the fused routes; launch_magnitude_in
and launch_render_bands have switches of their own.  The other GPU files reach those by a few named configurations and by chance.  Here
every inequality has a context on either side, every class its window under three palettes, and per context:

  route          stft_kernel, render_path bits 0 and 1, sgx_bands_fused and sgx_bands_peak_fused equal the restatement wherever it claims them
  pixels         sgx_render_mags on MADE magnitudes -- a ramp in log level across the bins times seeded noise (every bin distinct: a wrong tap
                 or weight shows), columns scaled from 20 dB below the dB range to 20 dB above it (every level, both clamps), one all-zero
                 column, one with l = 0 and r > 0 -- bit for bit against oracle.render_columns.  Seven base columns tiled to 2 * blocks + 3
                 columns (blocks: what the launcher starts on this device), so the persistent workgroups walk several columns with their
                 prefetch in flight; every column is compared
  bands          sgx_magnitude_in over the context's own rows on the base columns: exact against oracle.magnitude_in; sgx_render_bands on
                 them gives the pixels again
  from PCM       on W + 9 H samples of noise at amplitudes 1, 1e-2, 1e-4: sgx_render_batch is sgx_render_mags on the context's own
                 sgx_stft_batch rows, and the same bytes under SGX_FLAG_NO_FUSED_RENDER; sgx_bands_batch is sgx_magnitude_in on those rows

Nothing here has a tolerance.  A case is a chunk of contexts; every context of a chunk runs, and the case fails with the list of all that
failed.  Counts, wall times and the mutations this sweep was held against: profiles/r11_pixel_plans.txt.  Run with -m gpu on an MI355X."""
import os
import time

import numpy as np
import pytest

import oracle
import pixel_plans as pp

pytestmark = pytest.mark.gpu

CHUNKS = pp.chunks()
BUFFER = 128 << 20
AMPLITUDES = (1.0, 1e-2, 1e-4)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "gradients.npz")))


def made_magnitudes(cfg) -> np.ndarray:
    """[7][M][2] float32: columns 0 .. 4 a ramp in log level across the bins -- each a fifth of [min_db - 20, max_db + 20] -- times seeded
    noise in [1/2, 1) per channel; column 5 all zero; column 6 column 2 with l = 0"""
    M = cfg.M
    rng = np.random.default_rng([cfg.W, cfg.rows, 11])
    lo, hi = cfg.min_db - 20.0, cfg.max_db + 20.0
    step = (hi - lo) / 5.0
    base = np.zeros((7, M, 2), np.float32)
    for k in range(5):
        db = lo + step * (k + np.arange(M) / max(M - 1, 1))            # the level of l^2 + r^2 before the noise
        amp = 10.0 ** (db / 20.0) / np.sqrt(2.0)
        base[k] = (amp[:, None] * rng.uniform(0.5, 1.0, (M, 2))).astype(np.float32)
    base[6] = base[2]
    base[6, :, 0] = 0.0
    return base


def set_palette(eng, cfg, tables):
    """sets the context's palette; returns what oracle.render_columns takes for it (a table, or None after oracle.set_gradient_fn)"""
    p = cfg.palette
    if p.kind == "scheme":
        from oracle.gradients import CONTINUOUS
        eng.set_builtin_scheme(p.name, stereo=p.stereo)
        oracle.set_gradient_fn(CONTINUOUS[p.name])
        return None
    table = tables[p.name] if p.kind == "builtin" else pp.ramp(p.n)
    eng.set_gradient(table, stereo=p.stereo)
    return table


def sweep_one(torch, ctx, tables, n_cu, stats):
    """every check of one context; returns the list of failures (strings), empty when the context holds"""
    from spectrogram_rs_amd import SgxError, SpectrogramEngine
    cfg = ctx.cfg
    tag = ctx.name
    fails = []
    try:
        eng = SpectrogramEngine(cfg.sample_rate, device=0, **cfg.engine_kwargs())
    except SgxError as err:
        return [f"{tag}: refused: {err}"]
    split = None
    try:
        grad = set_palette(eng, cfg, tables)
        info = eng.info
        # ---- route first
        k = pp.stft_kernel(cfg)
        if k is not None and info.stft_kernel != k:
            return [f"{tag}: stft_kernel {info.stft_kernel}, expected {k}"]
        if info.total_samples_per_column != pp.row_table(cfg).n_samples or info.sample_rate_u32 != cfg.sr_u32:
            return [f"{tag}: {info.total_samples_per_column} samples per column at {info.sample_rate_u32} Hz, the restatement has "
                    f"{pp.row_table(cfg).n_samples} at {cfg.sr_u32}"]
        for bit, want in zip((1, 2), pp.render_bits(cfg, ctx.proof)):
            if want is not None and bool(info.render_path & bit) != bool(want):
                fails.append(f"{tag}: render_path {info.render_path}: bit {bit >> 1} expected {want}")
        for name, got, want in (("bands_fused", eng.bands_fused, pp.bands_fused(cfg)), ("bands_peak_fused", eng.bands_peak_fused, pp.bands_peak_fused(cfg))):
            if want is not None and bool(got) != bool(want):
                fails.append(f"{tag}: {name} {got}, expected {want}")
        if fails:
            return fails
        # ---- sgx_render_mags on made magnitudes
        base = made_magnitudes(cfg)
        kw = dict(R=cfg.rows, f_min=cfg.f_min, f_max=cfg.f_max, interp=cfg.interp, stereo=cfg.palette.stereo, min_db=cfg.min_db, max_db=cfg.max_db,
                  mode=cfg.lut_index_mode)
        ref = oracle.render_columns(base, cfg.sr_u32, grad, **kw)
        n_lut = None if cfg.palette.kind != "scheme" else 257       # (a callback gradient: any size but 256 -- kGeneric's class for sizing)
        blocks = pp.blocks_launched(cfg, ctx.seeded, n_cu, n_lut)
        cols = max(10, min(2 * blocks + 3, BUFFER // (cfg.M * 8), BUFFER // (cfg.rows * 4)))
        idx = torch.arange(cols, device="cuda") % 7
        base_dev, ref_dev = torch.from_numpy(base).cuda(), torch.from_numpy(ref).cuda()
        px = eng.render_mags(base_dev[idx].contiguous())
        torch.cuda.synchronize()
        bad = (px != ref_dev[idx]).reshape(cols, -1).any(dim=1)
        stats["columns"] += cols
        if bool(bad.any()):
            which = torch.nonzero(bad).flatten()
            first = int(which[0])
            rows_bad = np.flatnonzero((px[first].cpu().numpy() != ref[first % 7]).any(axis=1))
            fails.append(f"{tag}: render_mags: {int(bad.sum())} of {cols} columns differ from the oracle (base columns "
                         f"{sorted(set((which % 7).tolist()))}); column {first}: {len(rows_bad)} rows, the first at image row {rows_bad[0]}")
        # ---- sgx_magnitude_in over the context's own rows, sgx_render_bands on them
        edges = eng.bin_edges()
        ranges = np.stack([edges[:-1], edges[1:]], 1)
        bands = eng.magnitude_in(base_dev, ranges)
        got = bands.cpu().numpy()
        rows = range(cfg.rows) if cfg.rows <= 4096 else list(range(0, cfg.rows, 16)) + [cfg.rows - 1]
        for col in range(7):
            want = np.stack([oracle.magnitude_in(base[col], cfg.sr_u32, float(edges[py]), float(edges[py + 1]), cfg.interp) for py in rows])
            if not np.array_equal(got[col][list(rows)].view(np.uint32), want.view(np.uint32)):
                fails.append(f"{tag}: magnitude_in differs from the oracle on base column {col}")
        if not torch.equal(eng.render_bands(bands), ref_dev):
            fails.append(f"{tag}: render_bands on the bands is not the oracle's pixels")
        # ---- from PCM: the pixels and the bands of the context's own rows, fused or not
        if ctx.batch:
            split = SpectrogramEngine(cfg.sample_rate, device=0, **{**cfg.engine_kwargs(), "fused_render": False})
            set_palette(split, cfg, tables)
            n = cfg.W + 9 * cfg.H
            noise = torch.from_numpy(oracle.white_noise(n * cfg.channels, seed=cfg.W + cfg.rows)).cuda()
            for amp in AMPLITUDES:
                x = noise * amp
                own = eng.stft_batch(x)
                want = eng.render_mags(own.reshape(-1, cfg.M, 2))
                if not torch.equal(eng.render_batch(x).reshape(want.shape), want):
                    fails.append(f"{tag}: amplitude {amp}: render_batch is not render_mags on the context's own rows")
                if not torch.equal(split.render_batch(x).reshape(want.shape), want):
                    fails.append(f"{tag}: amplitude {amp}: render_batch under SGX_FLAG_NO_FUSED_RENDER differs")
                stats["frames"] += own.shape[0]
            own = eng.stft_batch(noise)
            want = eng.magnitude_in(own.reshape(-1, cfg.M, 2), ranges).reshape(own.shape[0], eng.pairs, cfg.rows, 2)
            for name, e in (("bands_batch", eng), ("bands_batch under SGX_FLAG_NO_FUSED_RENDER", split)):
                if not torch.equal(e.bands_batch(noise).view(torch.int32), want.view(torch.int32)):
                    fails.append(f"{tag}: {name} is not magnitude_in on the context's own rows")
        torch.cuda.synchronize()
        return fails
    except SgxError as err:
        return fails + [f"{tag}: {err}"]
    finally:
        oracle.set_gradient_fn(None)
        eng.close()
        if split is not None:
            split.close()


@pytest.mark.parametrize("chunk", list(CHUNKS))
def test_pixel_plans(torch_cuda, tables, chunk):
    t0 = time.perf_counter()
    n_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    stats = {"columns": 0, "frames": 0}
    fails = []
    classes = {}
    for ctx in CHUNKS[chunk]:
        fails += sweep_one(torch_cuda, ctx, tables, n_cu, stats)
        classes[ctx.cls] = classes.get(ctx.cls, 0) + 1
    print(f"PIXEL PLANS {chunk}: {len(CHUNKS[chunk])} contexts, {stats['columns']} columns, {stats['frames']} frames, "
          f"{time.perf_counter() - t0:.2f} s; classes {classes}")
    assert not fails, "\n".join([f"{len(fails)} failures in {chunk}:"] + fails)

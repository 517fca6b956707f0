"""The filterbank calls against the sum order that include/sgx.h makes part of the contract, bit for bit.

Every route runs one device body (csrc/sgx_fbank.hpp), so "fused == workspace == stage" compares that body with itself.  Here the
device meets tests/fbank_reference.py, written from the header's text: 64 fused-multiply-add chains from +0 over i = l, l + 64, ..., the
tree by halving, for the cross sums four products rounded without contraction.  tests/test_fbank_reference.py holds that reference to
libm's fmaf and shows that the banks and rows used here tell another tree, another lane stride and another filter's place apart, and that
no intermediate on the synthetic rows is denormal.  No tolerance appears in this file.

A disagreement is reported by route, filter, its (first, count), and the reference's partial sums per level of the tree."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as es
import fbank_reference as fr
from spectrogram_rs_amd import SpectrogramEngine, mel_weights

pytestmark = pytest.mark.gpu

SR = 48000.0
COLUMNS = 3
FUSED_MAX_FILTERS, FUSED_MAX_WEIGHTS = 1024, 16384      # include/sgx.h: sgx_fbank_fused

# the stage alone: name -> engine keyword arguments.  W 20481 | 20482 and 10241 | 10242 lie on either side of the stage kernels' decisions
# to hold the column in LDS (fbank_reference.stage_staged, cross_stage_staged)
STAGE_CONTEXTS = {
    "w64": dict(window_samples=64, hop_samples=16, channels=2),
    "w2048": dict(window_samples=2048, hop_samples=256, channels=2),
    "w2400_mono": dict(window_samples=2400, hop_samples=93),
    "w8192": dict(window_samples=8192, hop_samples=512, channels=2),
    "w10241": dict(window_samples=10241, hop_samples=5000, channels=2, large_transforms=True),
    "w10242": dict(window_samples=10242, hop_samples=5000, channels=2, large_transforms=True),
    "w20481": dict(window_samples=20481, hop_samples=10000, channels=2, large_transforms=True),
    "w20482": dict(window_samples=20482, hop_samples=10000, channels=2, large_transforms=True),
}
# (magnitude stage in LDS, cross stage in LDS) on a device with 160 KiB of opt-in LDS
STAGED = {"w64": (True, True), "w2048": (True, True), "w2400_mono": (True, True), "w8192": (True, True), "w10241": (True, True),
          "w10242": (True, False), "w20481": (True, False), "w20482": (False, False)}
FUSED_ROUTES = ["k1r_h256", "k1_lr_h256", "k1_ch4", "k48_lr"]
FUSED_FRAMES = 9


def lds_optin():
    hip = C.CDLL("libamdhip64.so")
    optin = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(optin), 75, 0) == 0      # hipDeviceAttributeSharedMemPerBlockOptin
    return optin.value


@functools.lru_cache(maxsize=None)
def banks(W):
    return {"edges": fr.edge_bank(W - 1), "mel128": mel_weights(SR, W, 128, 0.0, SR / 2)}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, x, bank, what):
    """got, want [..., n_filters, C]; x [..., M, C] the elements the reference summed"""
    g, w = u32(got), u32(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape}, expected {w.shape}"
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    idx = tuple(int(i) for i in bad[0])
    f, comp = idx[-2], idx[-1]
    levels = fr.filter_levels(x[idx[:-2]], bank, f) if bank[1][f] else []
    lines = [f"{what}: {len(bad)} of {g.size} words differ from the definition, in {len(set(map(int, bad[:, -2])))} filters",
             f"  first: column {idx[:-2]}, filter {f} (first {int(bank[0][f])}, count {int(bank[1][f])}), component {comp}: "
             f"device {float(got[idx])!r} ({int(g[idx]):#010x}), definition {float(want[idx])!r} ({int(w[idx]):#010x})"]
    elsewhere = np.flatnonzero(w[idx[:-2]][:, comp] == g[idx])
    if elsewhere.size:
        lines.append(f"  the device's value is the definition's for filter(s) {elsewhere.tolist()} of that column")
    for name, level in zip(["chains a[0..63]", "s = 32", "s = 16", "s = 8", "s = 4", "s = 2", "s = 1"], levels):
        lines.append(f"  {name}: {[float(v) for v in level[:, comp][:8]]}{' ...' if level.shape[0] > 8 else ''}")
    raise AssertionError("\n".join(lines))


# ---- the stage kernels on synthetic rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STAGE_CONTEXTS))
def test_stage_equals_the_definition(name):
    import torch

    eng = SpectrogramEngine(SR, device=0, **STAGE_CONTEXTS[name])
    try:
        M = eng.M
        assert M == STAGE_CONTEXTS[name]["window_samples"] - 1
        cap = lds_optin()
        assert cap >= fr.STAGE_LDS_CAP, f"this device offers {cap} bytes of LDS: the lengths here no longer lie on both sides of the decision"
        assert (fr.stage_staged(M, cap), fr.cross_stage_staged(M, cap)) == STAGED[name]
        mags = fr.synthetic_mags(COLUMNS, M, 101)
        spec = fr.synthetic_spec(COLUMNS, M, 102)
        assert fr.zero_or_normal(mags) and fr.zero_or_normal(spec)
        d_mags, d_spec = torch.from_numpy(mags).to(eng.device), torch.from_numpy(spec).to(eng.device)
        for kind, bank in banks(eng.W).items():
            got = {}
            for power in (1, 2):
                fb = eng.filterbank(*bank, power=power)
                got[power] = fb.apply(d_mags).cpu().numpy()
                if power == 2:
                    got["cross"] = fb.cross_apply(d_spec).cpu().numpy()
                fb.close()
            for power in (1, 2):
                assert_same_bits(got[power], fr.bank_sums(mags, bank, power), fr.elements(mags, power), bank, f"sgx_fbank_mags {name}/{kind}/power {power}")
            assert_same_bits(got["cross"], fr.cross_sums(spec, bank), fr.cross_elements(spec), bank, f"sgx_fbank_cross_spec {name}/{kind}")
            empty = bank[1] == 0
            assert (u32(got[2])[:, empty] == 0).all() and (u32(got["cross"])[:, empty] == 0).all()
    finally:
        eng.close()


# ---- the fused kernels end to end: PCM to sums against the definition over the engine's own rows -------------------------------------
@pytest.mark.parametrize("name", FUSED_ROUTES)
def test_batch_equals_the_definition_over_the_rows(name):
    import torch

    route = es.ROUTE[name]
    eng = SpectrogramEngine(SR, device=0, **route.engine_kwargs())
    try:
        assert eng.info.stft_kernel == route.kernel
        fused = 1 if route.kernel == 2 else 0
        pcm = eng.white_noise(eng.W + (FUSED_FRAMES - 1) * eng.H, seed=0x0FBA0DE5)
        rows = eng.stft_batch(pcm).cpu().numpy()
        assert rows.shape == (FUSED_FRAMES, eng.pairs, eng.M, 2)
        assert fr.zero_or_normal(rows) and (rows != 0).all(), f"{name}: a magnitude of the noise is zero or denormal"
        spec = None
        if eng.channels >= 2:
            spec = torch.view_as_real(eng.stft_batch_complex(pcm)).cpu().numpy()
            assert spec.shape == (FUSED_FRAMES, eng.pairs, eng.M, 2, 2)
            assert fr.zero_or_normal(spec), f"{name}: a word of the complex rows is denormal"

        def normal(a):
            assert fr.zero_or_normal(a), f"{name}: an intermediate of the definition is denormal on these rows"

        for kind, bank in banks(eng.W).items():
            assert len(bank[0]) <= FUSED_MAX_FILTERS and bank[2].size <= FUSED_MAX_WEIGHTS
            for power in (1, 2):
                fb = eng.filterbank(*bank, power=power)
                assert fb.fused == fused, f"{name}/{kind}: sgx_fbank_fused"
                got = fb.batch(pcm).cpu().numpy()
                assert_same_bits(got, fr.bank_sums(rows, bank, power, normal), fr.elements(rows, power), bank, f"sgx_fbank_batch {name}/{kind}/power {power}")
                if power == 2 and spec is not None:
                    assert fb.cross_fused == fused, f"{name}/{kind}: sgx_fbank_cross_fused"
                    got = fb.cross_batch(pcm).cpu().numpy()
                    assert_same_bits(got, fr.cross_sums(spec, bank, normal), fr.cross_elements(spec), bank, f"sgx_fbank_cross_batch {name}/{kind}")
                fb.close()
    finally:
        eng.close()

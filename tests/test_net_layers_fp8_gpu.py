"""GPU tests that hold EVERY LAYER of the "net_fp8" numerics class -- k_conv2_table_x8, k_gemm_ring_f8 and k_gemm_skinny_f8, and the
bf16 FCs and heads behind them -- to the float64 layer-by-layer reference of tests/net_layers_ref_fp8.py, element for element, with
bounds that are derived, not measured (that module's docstring; tests/test_net_layers_fp8_cpu.py shows that honest f32 kernels meet
them and that a dropped K-step, swapped taps or 16-byte chunks, a neighbour's dq or bias, the wrong scale, truncation, a wrong
board's rows or a shifted ragged tile do not).  tests/test_fp8_gpu.py compares conv3's codes at one width and (pi, v) end to end.

Every model is pinned with net_set_class(id, NET_CLASS_FP8) on a diagnostic engine; the readers are az_diag_read_conv2_out_fp8,
az_diag_read_conv3_out_fp8, az_diag_read_act (layers 4 / 5 / 6), az_diag_read_conv_table and az_diag_fp8_scales; the scales passed
to the reference are the engine's own.  az_net_predict_states with B <= max_batch runs ONE forward with the rows in the caller's
order, so workspace row i is state i.

  exact data   integer parameters (net_ref.exact_params): act2 and act3 codes and act4 / fc1 / fc2 bits must be the reference's at
               C = 128 / 256 / 384 / 512, at every row count around the kernels' hand-overs (ROWS), with "narrow_rows" 32 / 0 / 8192.
  random data  random_params, teacher-forced: conv2's codes from the device's own u2 rows bit for bit; conv3's codes from the
               device's act2 codes inside the accepted interval; conv4's bf16 from the device's act3 codes inside
               2^-8 relu(y) + beta; fc1, fc2 and the heads inside the bf16 module's bounds.  Every element.

Saturating activations are out of scope: the scales come from the weights alone with 4 x headroom, so no legal input reaches
+-448 (the reference asserts that the test data stay clear of it); tests/test_fp8_cpu.py covers the host quantiser's clamp.

Measured on the MI355X (information, not the bar: the bars are the interval and 1):
  exact data: no code and no bit differed, at any width, row count or "narrow_rows"; |dpi|, |dv| <= 6e-8.  Engine scales (sa2, sa3):
    1 / 0.125, 1 / 0.0625, 0.5 / 0.03125, 0.5 / 0.03125 at C = 128 / 256 / 384 / 512; largest scaled activations 54 .. 87.5 of 448.
  random data, 150 boards, "narrow_rows" 32 and 8192 (the same figures: the ring and the skinny kernel store the same bits):
    C = 128 (scales 32, 64): conv2 0 codes differ; conv3 0 outside the interval, 166 of 384000 codes (4.3e-4) off the nearest one,
      all one step away -- honest f32 (128-product blocks accumulated in f32) on the same device inputs: 0; share of elements with
      > 1 accepted code 0.0752, > 2 0.0141, nonzero 0.480; conv4 err / bound 0.791, 321 of 115200 bf16 values (2.8e-3) off the nearest
      one, 296 one step -- honest f32: 0; err / bound fc1 0.920 fc2 0.828 pi 4.3e-4 v 2.8e-4
    C = 512 (scales 64, 64): conv2 0; conv3 0 outside, 351 of 1536000 (2.3e-4) off the nearest code, 350 one step -- honest f32: 2;
      shares 0.3024 / 0.1034 / 0.496; conv4 err / bound 0.379, 1502 of 460800 (3.3e-3) off, 1369 one step -- honest f32: 7;
      err / bound fc1 0.544 fc2 0.804 pi 3.4e-4 v 4.0e-4
  700 boards at C = 512, the 64 boards of the subset: conv2 0; conv3 0 outside, 146 of 655360 (2.2e-4) off the nearest code, all one
      step -- honest f32: 1; conv4 err / bound 0.369, 649 of 196608 off, 592 one step -- honest f32: 4; fc1 0.527 fc2 0.767
  end to end against the emulation of tests/net_ref_fp8.py on the first 48 boards (C = 128 / 512): conv2 codes that differ 2 of
      258048 / 3 of 1032192; conv3 codes that differ 66 of 122880 / 153 of 491520, of which teacher-forcing on the same boards
      (identical inputs) already shows 55 / 108.
What the figures show: with bit-identical e4m3 inputs and weights the device stores a conv3 code one step off the nearest one in
2.2e-4 .. 4.3e-4 of the elements, where an f32 sum in any of three orders does so in at most 1.5e-6 -- so the one-step differences
are made by the summation inside v_mfma_f32_16x16x128_f8f6f4, which is less accurate than an f32 sum of the 128 exact products (by
the rates, an error of the order of 1e-5 of the value; still inside the worst-case f32 bound beta everywhere), not by the ORDER of
an f32 accumulation and not inherited from conv2: conv2's codes are the table's bit for bit, the emulation's conv2 differs in 3e-6 ..
8e-6 of the codes, and that accounts for the remaining sixth to third of the end-to-end differences.
"""
import ctypes

import numpy as np
import pytest
import torch

import net_layers_ref as L
import net_layers_ref_fp8 as L8
import net_ref_fp8 as r8
from net_ref import exact_params, random_params, unpack
from test_fp8_gpu import conv3_codes, fp8_scales
from test_net_gpu import random_states
from test_net_layers_gpu import read_act, read_u2_rows

pytestmark = pytest.mark.gpu

# Boards per forward of the exact-data test; conv3 has M = 20 n rows, conv4 M = 6 n.  k_gemm_skinny_f8 runs 1 x 1 tiles (16 x 16, ring
# depth 9) while ceil(M / 16) * (C / 16) <= 256 and 2 x 2 tiles (32 x 32, depth 6 at C = 256 / 512: <.., 9, 6>, depth 3 at C = 128 /
# 384: <.., 9, 3>) beyond; launch_gemm_f8 hands conv3 to the ring past "narrow_rows" boards and conv4 past twice as many; up to 150
# boards launch_ring_auto takes the one-workgroup-per-CU family k_gemm_ring_f8<.., 4, F8> (M <= 256 / (C / 128) * 96 at every width)
# and ring_pick_bm its 64-row tile (ceil(3000 / 64) * (C / 128) <= 256).  With "narrow_rows" = 32, per count (conv3 | conv4):
#     1                  1 x 1 | 1 x 1                     at every width (one ragged tile: 20 and 6 rows)
#     6, 7               C = 512: conv3 1 x 1 -> 2 x 2 (8 * 32 = 256 waves, then 9 * 32); 1 x 1 elsewhere | 1 x 1
#     8, 9               C = 384: conv3 1 x 1 -> 2 x 2 (10 * 24 = 240, then 12 * 24) | 1 x 1
#     12, 13             C = 256: conv3 1 x 1 -> 2 x 2 (15 * 16 = 240, then 17 * 16) | 1 x 1
#     21, 22             conv3 2 x 2 at 256 .. 512, 1 x 1 at 128 | C = 512: conv4 1 x 1 -> 2 x 2 (8 * 32, then 9 * 32)
#     25, 26             C = 128: conv3 1 x 1 -> 2 x 2 (32 * 8 = 256, then 33 * 8) | conv4 2 x 2 at 512, 1 x 1 elsewhere
#     26, 27             | C = 384: conv4 1 x 1 -> 2 x 2 (10 * 24, then 11 * 24)
#     32, 33             conv3 skinny 2 x 2 (640 rows) -> ring, 64-row tiles (660 rows, ragged) | conv4 skinny
#     42, 43             conv3 ring | C = 256: conv4 1 x 1 -> 2 x 2 (16 * 16, then 17 * 16); C = 128 stays on 1 x 1 (at most 24 * 8)
#     64, 65             conv3 ring | conv4 skinny (384 rows) -> ring, 64-row tiles (390 rows)
#     150                conv3 ring, 3000 rows = 46 tiles of 64 + 56 | conv4 ring, 900 rows = 14 tiles + 4
# "narrow_rows" = 0: the ring's 64-row tile at every count.  "narrow_rows" = 8192: the skinny kernel at every count, the same tile
# switches, up to 3000 and 900 rows on 2 x 2 tiles (93 full tiles + 24 rows; 28 + 4) -- at C = 128 conv4 leaves the 1 x 1 tiles only
# there (past 85 boards: 150).
ROWS = (1, 6, 7, 8, 9, 12, 13, 21, 22, 25, 26, 27, 32, 33, 42, 43, 64, 65, 150)
NARROW_ROWS = (32, 0, 8192)
ACT_NO = {"act4": 4, "fc1": 5, "fc2": 6}


def conv2_codes(e, rows, channels):
    """conv2's e4m3 output of the engine's last forward: rows x [6][7][C] codes."""
    f = e._lib.az_diag_read_conv2_out_fp8
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    out = np.empty((rows, 6, 7, channels), np.uint8)
    assert f(e._h, rows, out.ctypes.data_as(ctypes.c_void_p)) == out.nbytes
    return out


@pytest.fixture(scope="module")
def states(oracle):
    st = L.layer_states(random_states, oracle)
    assert st.shape == (150, 2) and not (st[:, 0] & st[:, 1]).any()
    return st


_EXACT = {}


def exact_reference(states, channels, sa2, sa3):
    """forward_exact on the 150 states, once per (width, scales) for the module; its conditions are asserted from the reference alone,
    and its f32 evaluation is the float64 one."""
    key = (channels, sa2, sa3)
    if key not in _EXACT:
        params = exact_params(channels, L.EXACT_SEED, L8.HEAD_SHIFT[channels])
        ref = L8.forward_exact(states, params, channels, sa2, sa3)
        L8.exact_conditions(ref)
        ref8 = L8.forward_exact(states[:8], params, channels, sa2, sa3, dtype=torch.float64)
        assert all(np.array_equal(ref8[k], ref[k][:8]) for k in ("act2", "act3", "act4", "fc1", "fc2"))
        _EXACT[key] = ref
    return _EXACT[key]


def read_layers(e, n, channels):
    out = {"act2": conv2_codes(e, n, channels), "act3": conv3_codes(e, n, channels)}
    for name, layer in ACT_NO.items():
        out[name] = read_act(e, layer, n, channels)
    return out


# ---- exact data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [128, 256, 384, 512])
def test_exact_data_every_layer_bit_for_bit(engine_mod, states, channels):
    """C = 128 and 384 take k_gemm_skinny_f8<.., 9, 3> and one / three ring column tiles, 256 and 512 <.., 9, 6> and two / four.  The row
    counts are prefixes of the 150 states of ONE reference; under each "narrow_rows" every layer's stored form equals the reference's,
    pi and v are within the 1e-6 left to exp / tanh and bit-equal across the three settings."""
    params = exact_params(channels, L.EXACT_SEED, L8.HEAD_SHIFT[channels])
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        e.net_set_params(0, params)
        e.net_set_class(0, engine_mod.NET_CLASS_FP8)
        sa2, sa3 = fp8_scales(e, 0)
        ref = exact_reference(states, channels, sa2, sa3)
        print(f"exact C={channels}: scales {sa2} {sa3}; largest scaled activations {ref['scaled_max']}; distinct act3 codes {np.unique(ref['act3']).size}")
        first = {}
        try:
            for nr in NARROW_ROWS:
                e.set_option("narrow_rows", nr)
                for n in ROWS:
                    pi, v = e.predict_states(states[:n], 0)
                    for name, got in read_layers(e, n, channels).items():
                        want = ref[name][:n].reshape(got.shape)
                        if not np.array_equal(got, want):
                            bad = np.argwhere(got != want)
                            raise AssertionError((channels, "narrow_rows", nr, "boards", n, "layer", name, "elements that differ", len(bad),
                                                  "first (board, position.., channel)", bad[:4].tolist(), "boards", np.unique(bad[:, 0])[:8].tolist(),
                                                  "channels", np.unique(bad[:, -1])[:8].tolist()))
                    assert np.abs(pi - ref["pi"][:n]).max() <= 1e-6 and np.abs(v - ref["v"][:n]).max() <= 1e-6, (nr, n)
                    if n not in first:
                        first[n] = (pi, v)
                    assert np.array_equal(pi, first[n][0]) and np.array_equal(v, first[n][1]), (nr, n)
        finally:
            e.set_option("narrow_rows", 32)
    finally:
        e.close()


# ---- random data, teacher-forced ----------------------------------------------------------------------------------------
def check_teacher_forced(e, model_id, params, states, channels, tag, subset=None, emulated=0):
    """One forward of `states`; for the boards of `subset` (all of them by default) every layer within its bound of the reference
    computed from the DEVICE's own input to that layer, every element.  Returns the figures it prints."""
    n = len(states)
    idx = np.arange(n) if subset is None else np.asarray(subset)
    sa2, sa3 = fp8_scales(e, model_id)
    pi, v = e.predict_states(states, model_id)
    assert np.isfinite(pi).all() and np.isfinite(v).all(), tag
    dev = {k: a[idx] for k, a in read_layers(e, n, channels).items()}
    assert all(len(a) == len(idx) for a in dev.values())                   # no board of the subset is skipped
    folded = L.fold_like_engine(params, channels)
    q = L8.quantised(params, channels, sa2, sa3)
    fig = {}
    # conv2: the gather over the device's own u2 rows, exactly
    pats = np.unique(L.patterns_of(states[idx]))
    u2 = read_u2_rows(e, model_id, pats, channels)
    lut = np.full(L.PATTERNS, -1)
    lut[pats] = np.arange(len(pats))
    want2, max2 = L8.conv2_codes_ref(lambda p: u2[lut[p]], states[idx], folded, sa2)
    assert max2 < L8.FP8_MAX and (want2 != 0).mean() > 0.1
    fig["conv2 codes that differ"] = int((dev["act2"] != want2).sum())
    # conv3: the interval, from the reference alone first
    y3, beta3, _ = L8.layer8_ref("conv3", L8.code_values(dev["act2"]), q)
    share, share2, alive = L8.nonvacuous(y3, beta3, sa3, L8.SHARE_CAP[channels])
    lo, hi = L8.accepted_codes(y3, beta3, sa3)
    near = L8.nearest_codes(y3, sa3)
    out3 = int((~L8.inside(dev["act3"], lo, hi)).sum())
    off, one = L8.off_nearest(dev["act3"], near)
    qw, dq, b, _ = q["conv3"]
    cpu3 = L8.store_conv3(L8.epilogue_f32(L8.acc_blocks_f32(L8.im2col("conv3", L8.code_values(dev["act2"])), qw, channels), dq, b), sa3)
    cpu_off, _ = L8.off_nearest(cpu3.reshape(near.shape), near)
    fig["conv3"] = (f"outside the interval {out3}, off the nearest code {off} of {near.size} ({one} one step away; honest f32 on the same inputs: "
                    f"{cpu_off}; equal to the honest f32 codes: {bool(np.array_equal(cpu3.reshape(near.shape), dev['act3']))}); "
                    f"> 1 accepted code {share:.4f}, > 2 {share2:.4f}, nonzero {alive:.3f}")
    # conv4: bf16
    y4, beta4, _ = L8.layer8_ref("conv4", L8.code_values(dev["act3"]), q)
    assert (y4 > 0).mean() > 0.1
    r4 = L.worst_ratio(L.bf16_from_bits(dev["act4"]), np.maximum(y4, 0.0), L8.conv4_bound(y4, beta4))
    d4 = dev["act4"].astype(int) - L.bf16_bits(np.maximum(y4, 0.0)).astype(int)
    qw4, dq4, b4, _ = q["conv4"]
    cpu4 = L.bf16_bits(L8.epilogue_f32(L8.acc_blocks_f32(L8.im2col("conv4", L8.code_values(dev["act3"])), qw4, channels), dq4, b4)).reshape(d4.shape)
    c4 = cpu4.astype(int) - L.bf16_bits(np.maximum(y4, 0.0)).astype(int)
    fig["conv4"] = (f"err / bound {r4:.3f}, bf16 values off the nearest one {int((d4 != 0).sum())} of {d4.size} ({int((np.abs(d4) == 1).sum())} one step away; "
                    f"honest f32 on the same inputs: {int((c4 != 0).sum())})")
    # fc1, fc2, heads: the bf16 module's bounds
    ratios = {}
    a = L.bf16_from_bits(dev["act4"])
    for name in ("fc1", "fc2"):
        y, S = L.layer_ref(name, a, folded)
        a = L.bf16_from_bits(dev[name])
        ratios[name] = L.worst_ratio(a.reshape(y.shape), y, L.bound_bf16(y, S, L.layer_k(name, channels)))
    rpi, rv, lb = L.heads_ref(a, folded)
    ratios["pi"] = float((np.abs(pi[idx] - rpi) / (0.5 * lb[:, None] + 1e-6)).max())
    ratios["v"] = float((np.abs(v[idx] - rv) / (lb + 1e-6)).max())
    fig["err / bound"] = " ".join(f"{k} {r:.3g}" for k, r in ratios.items())
    if emulated:
        # end to end against the whole-net emulation (tests/net_ref_fp8.py) on the first boards: what the codes inherit from the layers before
        k = min(emulated, len(idx))
        boards = L.boards_of(states[idx[:k]])
        with torch.no_grad():
            emu2 = r8.e4m3_codes(r8._front(unpack(np.asarray(params, np.float32), channels), torch.from_numpy(boards)) * np.float32(sa2)).permute(0, 2, 3, 1).numpy()
        emu3 = r8.forward_fp8(params, boards, channels, sa2, sa3, details=True)[2]["act3_codes"]
        fig["end to end, codes that differ from the emulation's"] = (f"conv2 {int((emu2 != dev['act2'][:k]).sum())} of {emu2.size}, conv3 {int((emu3 != dev['act3'][:k]).sum())} "
                                                                     f"of {emu3.size} (teacher-forced on these boards: {L8.off_nearest(dev['act3'][:k], near[:k])[0]})")
    print(f"teacher-forced fp8 C={channels} {tag} (scales {sa2} {sa3}, {len(idx)} boards): " + "; ".join(f"{k}: {x}" for k, x in fig.items()))
    if fig["conv2 codes that differ"]:
        bad = np.argwhere(dev["act2"] != want2)
        raise AssertionError((tag, "conv2 codes that differ", len(bad), "first (board, y, x, channel)", bad[:4].tolist()))
    if out3:
        bad = np.argwhere(~L8.inside(dev["act3"], lo, hi))
        raise AssertionError((tag, "conv3 codes outside their interval", out3, "first (board, y, x, channel)", bad[:4].tolist(),
                              "boards", idx[np.unique(bad[:, 0])][:8].tolist(), "channels", np.unique(bad[:, -1])[:8].tolist()))
    assert r4 <= 1, (tag, "conv4", r4)
    for k, r in ratios.items():
        assert r <= 1, (tag, k, r)
    return fig


@pytest.mark.parametrize("channels", [128, 512])
def test_random_data_every_layer_teacher_forced(engine_mod, states, channels):
    """150 states, random_params(C, 40 + C), the shipped rule ("narrow_rows" 32: both layers on the ring's one-per-CU family) and the
    skinny kernel alone (8192: 3000 and 900 rows on 2 x 2 tiles)."""
    params = random_params(channels, seed=40 + channels)
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=channels, diag=True)
    try:
        e.net_set_params(1, params)
        e.net_set_class(1, engine_mod.NET_CLASS_FP8)
        try:
            for nr in (32, 8192):
                e.set_option("narrow_rows", nr)
                check_teacher_forced(e, 1, params, states, channels, f"narrow_rows {nr}", emulated=48 if nr == 32 else 0)
        finally:
            e.set_option("narrow_rows", 32)
    finally:
        e.close()


def test_random_data_large_batch_teacher_forced(engine_mod, oracle):
    """700 boards at C = 512 (max_batch 1024): conv3's 14000 rows run k_gemm_ring_f8<2, 2, 1> (two workgroups per CU, 128-row tiles),
    conv4's 4200 rows the one-per-CU family's 96-row tile.  The reference is computed for 64 boards -- the first 12, the last 12 and 40
    drawn from the rest with seed 7; tests/test_fp8_gpu.py::test_fp8_rows_depend_on_their_state_alone ties every other row count
    and row to these bit for bit."""
    channels, n = 512, 700
    params = random_params(channels, seed=40 + channels)
    st = random_states(oracle, n, seed=100 + n)
    subset = np.concatenate([np.arange(12), np.sort(np.random.default_rng(7).choice(np.arange(12, n - 12), 40, replace=False)), np.arange(n - 12, n)])
    assert len(np.unique(subset)) == 64
    e = engine_mod.Engine(device=0, max_batch=1024, net_channels=channels, diag=True)
    try:
        e.net_set_params(1, params)
        e.net_set_class(1, engine_mod.NET_CLASS_FP8)
        check_teacher_forced(e, 1, params, st, channels, "700 boards", subset=subset)
    finally:
        e.close()

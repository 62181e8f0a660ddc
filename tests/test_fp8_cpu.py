"""The "net_fp8" numerics class without a GPU: the C++ quantiser (csrc/az_fp8.h, built with g++) against torch.float8_e4m3fn, its
scale rules and packed-copy index math against a plain restatement, and the error budget of the scheme itself
(tests/net_ref_fp8.py against the textbook f32 net)."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero-rs_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from net_ref import forward_ref, random_params      # noqa: E402
import net_ref_fp8 as r8                             # noqa: E402


@pytest.fixture(scope="module")
def quant(tmp_path_factory):
    d = tmp_path_factory.mktemp("fp8")
    exe = str(d / "test_fp8_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_fp8_cpu.cpp"), "-o", exe])

    def run(mode, arr=None, arg=None, dtype=np.uint8):
        out = str(d / "out.bin")
        cmd = [exe, mode]
        if arr is not None:
            inp = str(d / "in.bin")
            np.ascontiguousarray(arr).tofile(inp)
            cmd.append(inp)
        if arg is not None:
            cmd.append(str(arg))
        subprocess.check_call(cmd + [out])
        return np.fromfile(out, dtype=dtype)
    return run


def _torch_codes(x):
    return torch.from_numpy(x).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_all_256_codes_round_trip(quant):
    vals = quant("decode", dtype=np.float32)
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert np.array_equal(np.isnan(vals), np.isnan(ref)) and int(np.isnan(vals).sum()) == 2          # 0x7F, 0xFF: e4m3fn has no infinity
    ok = ~np.isnan(ref)
    assert np.array_equal(vals[ok].view(np.uint32), ref[ok].view(np.uint32))                          # -0 included
    assert vals[0x7E] == 448.0 and vals[0x01] == 2.0 ** -9 and vals[0x08] == 2.0 ** -6
    codes = quant("quant", vals[ok])
    assert np.array_equal(codes, np.arange(256, dtype=np.uint8)[ok])


def test_quantiser_matches_torch_on_a_dense_sweep(quant):
    """Every code's value, every midpoint between neighbouring codes (the ties) and their f32 neighbours on both sides, the subnormal
    range down to f32 subnormals, +-448 and its neighbours, and 200,000 random values over the whole range."""
    grid = np.sort(torch.arange(0, 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy())
    mids = (grid[:-1] + grid[1:]) / 2
    pts = np.concatenate([grid, mids, [2.0 ** -10, 2.0 ** -11, 1e-30, 1e-40, 1e-45, 447.99, 463.9, 432.0, 440.0]]).astype(np.float32)
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))])
    rng = np.random.default_rng(0)
    rnd = np.concatenate([rng.uniform(-448, 448, 100000), rng.standard_normal(50000) * 0.05,
                          np.exp2(rng.uniform(-14, 9, 50000)) * rng.choice([-1.0, 1.0], 50000)]).astype(np.float32)
    x = np.concatenate([pts, -pts, rnd])
    x = x[np.abs(x) <= 448.0]
    assert np.array_equal(quant("quant", x), _torch_codes(x))
    assert len(x) > 200000


def test_values_beyond_448_saturate(quant):
    x = np.array([448.0, 448.0001, 464.0, 480.0, 1e4, 3e38, np.inf], np.float32)
    assert np.all(quant("quant", x) == 0x7E) and np.all(quant("quant", -x) == 0xFE)
    assert quant("quant", np.array([np.nan], np.float32))[0] & 0x7F == 0x7F


def _pow2_scale_plain(amax):
    """The largest power of two s with amax * s <= 448, by exact rational arithmetic."""
    if amax == 0:
        return 1.0
    a, k = Fraction(float(amax)), 0
    while a * Fraction(2) ** k <= 448:
        k += 1
    while a * Fraction(2) ** k > 448:
        k -= 1
    return float(Fraction(2) ** k)


def test_scale_rules(quant):
    rng = np.random.default_rng(1)
    amax = np.concatenate([[0.0, 448.0, 224.0, 447.99, 448.01, 1.0, 0.875, 0.8750001, 7.0, 3.5, 1e-6, 112.0, 111.99, 112.01, 56.0],
                           np.exp2(rng.uniform(-20, 12, 2000)), np.exp2(np.arange(-20, 12)), 448.0 * np.exp2(np.arange(-20, 4))]).astype(np.float32)
    out = quant("scales", amax, dtype=np.float32).reshape(-1, 2)
    for a, (sw, sa) in zip(amax.tolist(), out.tolist()):
        assert sw == _pow2_scale_plain(a), a
        assert sa == _pow2_scale_plain(4.0 * a), a
        assert sw == r8.pow2_scale(a) and sa == r8.act_scale(a), a            # the emulation's own restatement
        if a > 0:
            assert a * sw <= 448.0 < 2 * a * sw and math.log2(sw) == int(math.log2(sw))


def test_packed_copy_index_math(quant):
    """fp8_ring_offset against the layout's definition: [column tile][channel block][tap][row][16-byte slot = chunk ^ (row & 7)][byte],
    a bijection onto 9 C^2 bytes."""
    C = 256
    off = quant("offsets", arg=C, dtype=np.int64).reshape(C, 9, C)
    n, tap, c = np.meshgrid(np.arange(C), np.arange(9), np.arange(C), indexing="ij")
    nt, r, cb, cc = n // 128, n % 128, c // 128, c % 128
    want = ((((nt * (C // 128) + cb) * 9 + tap) * 128 + r) * 8 + ((cc // 16) ^ (r & 7))) * 16 + cc % 16
    assert np.array_equal(off, want)
    assert np.array_equal(np.sort(off.reshape(-1)), np.arange(9 * C * C))


def _legal_boards(n, seed):
    """Legal Connect Four positions at random depths as [n,2,6,7] planes (side to move first), no engine and no oracle needed."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 2, 6, 7), np.float32)

    def won(p):
        for y in range(6):
            for x in range(7):
                for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
                    if all(0 <= y + i * dy < 6 and 0 <= x + i * dx < 7 and p[y + i * dy, x + i * dx] for i in range(4)):
                        return True
        return False
    for b in range(n):
        planes, h = np.zeros((2, 6, 7), bool), [0] * 7
        for ply in range(int(rng.integers(0, 30))):
            a = int(rng.choice([c for c in range(7) if h[c] < 6]))
            nxt = planes.copy()
            nxt[0, 5 - h[a], a] = True
            if won(nxt[0]) or ply == 41:
                break
            planes = nxt[::-1].copy()
            h[a] += 1
        out[b] = planes
    return out


def _distance(params, boards, C, shrink=1.0):
    sa2, sa3 = r8.calibrate_scales(params, boards, C)
    pi, v = r8.forward_fp8(params, boards, C, sa2 / shrink, sa3 / shrink)
    fpi, fv = forward_ref(params, boards, C, emulate_bf16=False)
    return float(np.abs(pi - fpi).max()), float(np.abs(v - fv).max()), pi, v


def test_scheme_error_budget():
    """The emulation's distance from the textbook f32 net, measured here at C = 512 on 200 legal positions as the yardstick
    (seed 1: |dpi| 6.1e-3, |dv| 2.6e-2; seed 3: 3.7e-3, 2.3e-2 -- ten times the bf16 emulation's 5.9e-4 / 2.7e-3).  At C = 128 the
    distance must stay below twice the larger of those (measured 2.2e-3 / 1.9e-2 and 3.4e-3 / 2.2e-2), and activation scales 64 times
    smaller must move the result by less than a quarter of it (measured 5.0e-4 / 2.5e-3 and 5.4e-4 / 4.9e-3)."""
    boards = _legal_boards(200, seed=11)
    big = [_distance(random_params(512, seed), boards, 512)[:2] for seed in (1, 3)]
    print("C=512 fp8 emulation vs f32:", big)
    bar_pi, bar_v = max(b[0] for b in big), max(b[1] for b in big)
    for seed in (1, 3):
        p = random_params(128, seed)
        dpi, dv, pi, v = _distance(p, boards, 128)
        print("C=128 seed", seed, "fp8 emulation vs f32:", dpi, dv)
        assert dpi < 2 * bar_pi and dv < 2 * bar_v, (seed, dpi, dv, big)
        _, _, pi64, v64 = _distance(p, boards, 128, shrink=64.0)
        mpi, mv = float(np.abs(pi64 - pi).max()), float(np.abs(v64 - v).max())
        print("C=128 seed", seed, "scales / 64 move the result by:", mpi, mv)
        assert mpi < 0.25 * bar_pi and mv < 0.25 * bar_v, (seed, mpi, mv, big)

"""Torch emulation of the "net_fp8" numerics class (include/az_engine.h) on the CPU, built on net_ref.py.

conv1 and conv2 with the rounding of the engine's table kernels (_front), conv2's ReLU output stored as e4m3(x * sa2); conv3 and conv4
multiply e4m3 activations with per-output-channel-scaled e4m3 weights (products exact, the sum rounded to f32), undo both scales with
one exact power of two, add the f32 bias and apply ReLU; conv3's result is stored as e4m3(x * sa3), conv4's as bf16.  The FCs and heads are the
bf16 emulation's.  The activation scales are ARGUMENTS: the engine's come from its calibration set, a test passes what the engine
reports (or calibrates on its own inputs with calibrate_scales).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from net_ref import BN_EPS, bf16_round, unpack

FP8_MAX = 448.0
ACT_HEADROOM = 4.0


def e4m3(t):
    """f32 -> OCP e4m3fn -> f32: clamp to +-448, then round to nearest even."""
    return t.clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).to(torch.float32)


def e4m3_codes(t):
    return t.clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def pow2_scale(amax):
    """2^floor(log2(448 / amax)): the largest power of two s with amax * s <= 448; 1 for amax == 0."""
    amax = float(amax)
    if not (amax > 0.0) or math.isinf(amax):
        return 1.0
    m, e = math.frexp(amax)                 # 448 = 0.875 * 2^9
    return math.ldexp(1.0, 9 - e if m <= 0.875 else 8 - e)


def act_scale(amax):
    return pow2_scale(ACT_HEADROOM * float(amax))


def _fold(w, b, bn):
    gamma, beta, mean, var = bn[0], bn[1], bn[2], bn[3]
    s = gamma / torch.sqrt(var + np.float32(BN_EPS))
    return w * s, b * s + (beta - mean * s)


def weight_scales(wf):
    """wf [3][3][cin][cout] folded f32 -> sw [cout]"""
    amax = wf.abs().reshape(-1, wf.shape[-1]).amax(dim=0)
    return torch.tensor([pow2_scale(a) for a in amax.tolist()], dtype=torch.float32)


def _front(P, x):
    """conv1 + conv2 up to conv2's ReLU (f32, not yet rounded), with the rounding of the engine's TABLE kernels ("conv2_table" = 1, which
    the fp8 class requires), because one e4m3 step is 2^-4 and every earlier rounding that differs can move one:
      conv1  the bias, then the weights of the occupied cells added one by one in (ky, kx, plane) order in f32 -- k_conv1_table's own
             order, reproduced exactly (adding a weight times a 0 / 1 plane adds the weight or +-0) -- ReLU, bf16;
      conv2  each filter tap's sum over the input channels rounded to f16 (an entry of the per-model table; summed here in float64 so
             that the reference adds no order noise of its own), the nine taps added in (ky, kx) order in f32, then the bias."""
    wf, bf = _fold(P["conv1_w"], P["conv1_b"], P["conv1_bn"])
    xp = F.pad(x, (1, 1, 1, 1))
    a = bf.view(1, -1, 1, 1).expand(x.shape[0], -1, 6, 7).clone()
    for ky in range(3):
        for kx in range(3):
            for ci in range(2):
                a = a + wf[ky, kx, ci].view(1, -1, 1, 1) * xp[:, ci:ci + 1, ky:ky + 6, kx:kx + 7]
    x = bf16_round(torch.relu(a))
    wf, bf = _fold(P["conv2_w"], P["conv2_b"], P["conv2_bn"])
    wf = bf16_round(wf).double()
    xp = F.pad(x, (1, 1, 1, 1)).double()
    acc = torch.zeros(x.shape[0], wf.shape[3], 6, 7)
    for ky in range(3):
        for kx in range(3):
            w1 = wf[ky, kx].t().contiguous()[:, :, None, None]                  # [cout][cin][1][1]
            acc = acc + F.conv2d(xp[:, :, ky:ky + 6, kx:kx + 7], w1).float().to(torch.float16).to(torch.float32)
    return torch.relu(acc + bf.view(1, -1, 1, 1))


def calibrate_scales(params, boards, C):
    """(sa2, sa3) by the engine's rule from the bf16 path's conv2 / conv3 outputs on `boards`."""
    P = unpack(np.asarray(params, np.float32), C)
    x = torch.from_numpy(np.asarray(boards, np.float32).reshape(-1, 2, 6, 7))
    with torch.no_grad():
        a2 = bf16_round(_front(P, x))
        wf, bf = _fold(P["conv3_w"], P["conv3_b"], P["conv3_bn"])
        a3 = bf16_round(torch.relu(F.conv2d(a2, bf16_round(wf).permute(3, 2, 0, 1).contiguous(), bf)))
    return act_scale(a2.max().item()), act_scale(a3.max().item())


def forward_fp8(params, boards, C, sa2, sa3, details=False):
    """boards [B,2,6,7] f32 -> (pi [B,7], v [B]); details=True adds a dict with conv3's e4m3 codes as [B][4][5][C] uint8
    (the engine's act3 layout) and the largest scaled activation before the clamps."""
    P = unpack(np.asarray(params, np.float32), C)
    x = torch.from_numpy(np.asarray(boards, np.float32).reshape(-1, 2, 6, 7))
    sa2, sa3 = np.float32(sa2), np.float32(sa3)
    info = {}
    with torch.no_grad():
        y2 = _front(P, x) * sa2
        q = e4m3(y2)
        sa_in = sa2
        for l, sa_out in ((3, sa3), (4, None)):
            wf, bf = _fold(P[f"conv{l}_w"], P[f"conv{l}_b"], P[f"conv{l}_bn"])
            sw = weight_scales(wf)
            qw = e4m3(wf * sw)
            # e4m3 x e4m3 products are exact; summed in float64 and rounded to f32 ONCE, so that the reference carries no summation-order
            # noise of its own (the engine's f32 order inside the MFMA is its own; an f32 sum here would add a second, unrelated one)
            acc = F.conv2d(q.double(), qw.permute(3, 2, 0, 1).contiguous().double()).float()
            dq = (1.0 / (sw * sa_in)).to(torch.float32)
            y = torch.relu(acc * dq.view(1, -1, 1, 1) + bf.view(1, -1, 1, 1))
            if sa_out is not None:
                y3 = y * sa_out
                q = e4m3(y3)
                info["act3_codes"] = e4m3_codes(y3).permute(0, 2, 3, 1).contiguous().numpy()
                info["max_scaled"] = (float(y2.max()), float(y3.max()))
                sa_in = sa_out
            else:
                x = bf16_round(y)
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        for l in range(2):
            wf, bf = _fold(P[f"fc{l+1}_w"], P[f"fc{l+1}_b"], P[f"fc{l+1}_bn"])
            x = bf16_round(torch.relu(x @ bf16_round(wf) + bf))
        pi = torch.softmax(x @ P["pi_w"] + P["pi_b"], dim=1)
        v = torch.tanh(x @ P["v_w"] + P["v_b"]).reshape(-1)
    if details:
        return pi.numpy(), v.numpy(), info
    return pi.numpy(), v.numpy()

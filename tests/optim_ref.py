"""Float64 restatement of the trainer's opt-in optimiser rules (csrc/az_optim.h; include/az_engine.h "train_weight_decay_e9" ...): the
learning-rate table, the clip factor, which parameters decay, and the AdamW + EMA replay from a list of device-reported gradients.
Independent of the engine: numpy and net_ref.layout only."""
import math

import numpy as np

from net_ref import layout

NONE, COSINE, LINEAR = 0, 1, 2


def lr_at(lr, t, warmup, total, mode, floor):
    """f32 learning rate of applied step t (1-based): lr * warm * dec in double, rounded once."""
    lr = float(np.float32(lr))
    warm = min(1.0, t / warmup) if warmup > 0 else 1.0
    dec = 1.0
    if mode != NONE and total != 0:
        x = min(1.0, max(0.0, (t - warmup) / max(1, total - warmup)))
        if mode == COSINE:
            dec = floor + (1.0 - floor) * (0.5 * (1.0 + math.cos(math.pi * x)))
        else:
            dec = floor + (1.0 - floor) * (1.0 - x)
    return np.float32((lr * warm) * dec)


def lr_table(lr, steps, warmup, total, mode, floor):
    return np.array([lr_at(lr, t, warmup, total, mode, floor) for t in range(1, steps + 1)], np.float32)


def clip_scale(norm, c):
    """torch.nn.utils.clip_grad_norm_'s factor, f32."""
    with np.errstate(all="ignore"):
        r = np.float64(c) / (np.float64(norm) + 1e-6)
    return np.float32(r if (r < 1.0 or r != r) else 1.0)


def masks(C):
    """(decays, trainable) boolean masks over the flat parameter vector: the weight tensors decay; everything but BatchNorm's moving
    averages is the optimiser's."""
    off, total = layout(C)
    decays, trainable = np.zeros(total, bool), np.ones(total, bool)
    for k, (o, shp) in off.items():
        n = int(np.prod(shp))
        if k.endswith("_w"):
            decays[o:o + n] = True
        if k.endswith("_bn"):
            trainable[o + 2 * shp[1]:o + 4 * shp[1]] = False
    return decays, trainable


def segment_edges(C):
    """Every index at which the class of an element can change, and its neighbours: both edges of every segment."""
    off, total = layout(C)
    idx = set()
    for k, (o, shp) in off.items():
        n = int(np.prod(shp))
        cuts = [o, o + n] + ([o + q * shp[1] for q in (1, 2, 3)] if k.endswith("_bn") else [])     # gamma | beta | mean | variance
        for c in cuts:
            idx.update(i for i in (c - 1, c) if 0 <= i < total)
    return sorted(idx)


def replay(p0, grads, C, lr=1e-3, wd=0.0, clip=0.0, warmup=0, total=0, mode=NONE, floor=0.0, ema=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """AdamW (torch.optim.AdamW's decoupled decay in front of torch.optim.Adam's update) on the RAW gradients of each applied step, in
    float64 -> (weights, shadow or None, [(norm, scale, lr_t)]).  wd and ema are the f32 values the device holds."""
    decays, trainable = masks(C)
    wd, ema = float(np.float32(wd)), float(np.float32(ema))
    q = p0.astype(np.float64).copy()
    m, v = np.zeros_like(q), np.zeros_like(q)
    s = q.copy() if ema > 0 else None
    info = []
    for t, g in enumerate(grads, start=1):
        g = g.astype(np.float64)
        norm = float(np.sqrt(np.sum(g * g)))
        scale = float(clip_scale(norm, clip)) if clip > 0 else 1.0
        lr_t = float(lr_at(lr, t, warmup, total, mode, floor))
        g = g * scale
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        q[decays] *= 1.0 - lr_t * wd
        q -= (lr_t / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
        if s is not None:
            s[trainable] = ema * s[trainable] + (1 - ema) * q[trainable]
        info.append((norm, scale, lr_t))
    return q, s, info

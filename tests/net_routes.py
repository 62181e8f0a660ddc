"""The inference forward's kernel routes as pure functions, and the (n, rows_hint, rows_typ) triples that stand on both sides of
every line between two routes (tests/test_net_routes_cpu.py checks this module against itself and against the constants in the
text of csrc/az_net.hip; tests/test_net_routes_gpu.py runs the triples).

convnet_forward is handed three numbers: n, the exact row count, read on the device from EvalBatch::n; rows_hint, the host's upper
bound, which sizes the grids; rows_typ, the host's estimate (the previous move's largest batch), which picks kernel families.  It
first clamps the estimate -- rows_typ <= 0 or > rows_hint becomes rows_hint (norm_typ) -- so no launcher ever sees "no estimate".

The lines, per layer (rps = output rows per board: conv3 20, conv4 6, the FCs 1; ncol = N / GBN column tiles):

  skinny hand-over   launch_gemm / launch_gemm_f8: lim = narrow_rows x 1 / 2 / 4 / 4 boards for conv3 / conv4 / fc1 / fc2 (fp8: conv3
                     and conv4 only).  The skinny kernel is launched iff rows_typ <= 16 lim, alone iff rows_hint <= lim; beside a
                     tiled kernel it runs iff n <= lim (m_max) and the tiled one iff n > lim (m_min).  Inside it, 1 x 1 tiles while
                     ceil(n rps / 16) (N / 16) <= SK_SMALL_WAVES, 2 x 2 beyond.
  conv3 family       bf16: the ring's one-per-CU family (forced) iff rows_typ * 115 / 100 * 20 <= 8192, else the image-resident kernel.
  conv3 tail         image kernel: wid = ceil8(ceil(n / C3_NB)) (C / 128) workgroup ids; the last round's tiles are cut in two iff
                     0 < wid % 512 <= C3_TAIL.  The device decides from n; the host sizes full_grid from rows_hint.
  ring family        launch_ring_auto: m_one = 256 / ncol * (96 conv, 128 FC) rows.  An FC whose bound exceeds m_one and whose
                     estimate * 115 / 100 lies in [0.7, 1.4] m_one launches BOTH families (the window): one-per-CU runs iff
                     n rps <= m_one (m_hi), two-per-CU iff above (m_min).  Otherwise one-per-CU iff the bound fits m_one or the
                     estimate fits one round of the largest tile.
  ring tile          ring_pick_bm, on the device from n: one-per-CU 64 / 96 / 128 rows by whole-round fit; two-per-CU FC 96 / 128;
                     two-per-CU conv the cost rule over 96 / 128 / 160 / 192.
"""
import functools

import numpy as np

# ---- the constants the lines rest on (test_net_routes_cpu.py reads the same values from the source text) -------------------
C3_NB = 12
C3_TAIL = 128
GBN = 128
SK_SMALL_WAVES = 256
NARROW_ROWS = 32                       # the option's default
SKINNY_MULT = {"conv3": 1, "conv4": 2, "fc1": 4, "fc2": 4}
SKINNY_EST_FACTOR = 16                 # launched iff rows_typ <= 16 * lim
EST_NUM, EST_DEN = 115, 100            # the estimate + 15 %
CONV3_SMALL_ROWS = 8192                # conv3_is_small: (estimate + 15 %) * 20 <= 8192
WINDOW_LO, WINDOW_HI = 70, 140         # the FC window, per cent of m_one
MAX_BATCH = 8192
RPS = {"conv3": 20, "conv4": 6, "fc1": 1, "fc2": 1}
LAYERS = ("conv3", "conv4", "fc1", "fc2")
SHIPPED = {"narrow_rows": NARROW_ROWS, "conv3_small": 1, "conv3_tail": 1}
ALWAYS_N = (1, 12, 13, 96, 97, MAX_BATCH)


def width_n(layer, C):
    return {"conv3": C, "conv4": C, "fc1": 1024, "fc2": 512}[layer]


def norm_typ(rows_hint, rows_typ):
    """convnet_forward's clamp of the estimate."""
    return rows_hint if rows_typ <= 0 or rows_typ > rows_hint else rows_typ


def pow2_up(x):
    p = 1
    while p < x:
        p *= 2
    return p


# ---- skinny ---------------------------------------------------------------------------------------------------------
def skinny_lim(layer, cls, narrow_rows=NARROW_ROWS):
    """Boards up to which the skinny kernel takes the batch (0: "narrow_rows" is off).  The fp8 class has kernels of its own for conv3
    and conv4 (launch_gemm_f8) with the same multipliers; its FCs are the bf16 ones."""
    return max(narrow_rows, 0) * SKINNY_MULT[layer]


def skinny_launched(layer, cls, rows_hint, rows_typ, narrow_rows=NARROW_ROWS):
    lim = skinny_lim(layer, cls, narrow_rows)
    return lim > 0 and norm_typ(rows_hint, rows_typ) <= SKINNY_EST_FACTOR * lim


def skinny_tile(layer, C, n):
    """1: 16 x 16 tiles, 2: 32 x 32."""
    N = width_n(layer, C)
    return 1 if (n * RPS[layer] + 15) // 16 * (N // 16) <= SK_SMALL_WAVES else 2


# ---- conv3 ----------------------------------------------------------------------------------------------------------
def conv3_is_small(rows_hint, rows_typ):
    return norm_typ(rows_hint, rows_typ) * EST_NUM // EST_DEN * RPS["conv3"] <= CONV3_SMALL_ROWS


def conv3_wid(n, C):
    return ((n + C3_NB - 1) // C3_NB + 7) // 8 * 8 * (C // 128)


def conv3_cut(n, C, tail=1):
    rem = conv3_wid(n, C) % 512
    return bool(tail) and 0 < rem <= C3_TAIL


def conv3_grid(rows_hint, C, tail=1):
    """(full_grid, extra workgroups) the host launches."""
    return conv3_wid(rows_hint, C), C3_TAIL if tail else 0


# ---- the ring -------------------------------------------------------------------------------------------------------
def ring_pick_bm(M, ncol, ns, conv):
    """ring_pick_bm of csrc/az_net.hip, f32 where it is f32."""
    def wgs(bm):
        return (M + bm - 1) // bm * ncol
    if ns == 4:
        return 64 if wgs(64) <= 256 else 96 if wgs(96) <= 256 else 128
    if not conv:
        return 96 if wgs(96) <= 512 else 128
    f = np.float32
    best, best_cost = 128, f(1e30)
    for bm in range(96, 193, 32):
        w = wgs(bm)
        full, rem = w // 512, w % 512
        cost = f(f(10.0) + f(f(0.42) * f(bm))) * f(f(full) + (f(0.0) if rem == 0 else f(0.6) if rem <= 256 else f(1.0)))
        if cost < best_cost:
            best_cost, best = cost, bm
    return best


def ring_m_one(layer, C):
    conv = layer in ("conv3", "conv4")
    return 256 // (width_n(layer, C) // GBN) * (96 if conv else 128)


def ring_family(layer, C, rows_hint, rows_typ, force_one=False):
    """"one" (NS = 4, one workgroup per CU), "two" (NS = 2) or "window" (both launched, the device decides)."""
    conv = layer in ("conv3", "conv4")
    rps, ncol = RPS[layer], width_n(layer, C) // GBN
    tile_max, m_one = (96 if conv else 128), ring_m_one(layer, C)
    m_est, m_bound = norm_typ(rows_hint, rows_typ) * EST_NUM // EST_DEN * rps, rows_hint * rps
    if not force_one and not conv and m_bound > m_one and m_one * WINDOW_LO <= m_est * 100 <= m_one * WINDOW_HI:
        return "window"
    return "one" if force_one or m_bound <= m_one or (m_est + tile_max - 1) // tile_max * ncol <= 256 else "two"


def ring_kernel(layer, C, n, family):
    """(NS, tile rows) of the ring kernel that runs a batch of n boards."""
    conv = layer in ("conv3", "conv4")
    M, ncol = n * RPS[layer], width_n(layer, C) // GBN
    ns = {"one": 4, "two": 2}.get(family) or (4 if M <= ring_m_one(layer, C) else 2)
    return ns, ring_pick_bm(M, ncol, ns, conv)


# ---- one forward's route ----------------------------------------------------------------------------------------------
def route(cls, C, n, rows_hint, rows_typ, opts=None):
    """{layer: what runs}: ("skinny", tile, alone), ("ring", NS, rows, family, beside a skinny launch) or ("image", cut, extra
    workgroups that have work, beside a skinny launch).  cls: "bf16" or "fp8"."""
    o = {**SHIPPED, **(opts or {})}
    assert 1 <= n <= rows_hint and rows_typ >= 0
    out = {}
    for layer in LAYERS:
        lim = skinny_lim(layer, cls if layer in ("conv3", "conv4") else "bf16", o["narrow_rows"])
        beside = skinny_launched(layer, cls, rows_hint, rows_typ, o["narrow_rows"])
        if beside and (rows_hint <= lim or n <= lim):
            out[layer] = ("skinny", skinny_tile(layer, C, n), rows_hint <= lim)
            continue
        if layer == "conv3" and cls == "bf16":
            if o["conv3_small"] and conv3_is_small(rows_hint, rows_typ):
                out[layer] = ("ring",) + ring_kernel(layer, C, n, "one") + ("one", beside)
            else:
                out[layer] = ("image", conv3_cut(n, C, o["conv3_tail"]), beside)
            continue
        fam = ring_family(layer, C, rows_hint, rows_typ)
        out[layer] = ("ring",) + ring_kernel(layer, C, n, fam) + (fam, beside)
    return out


def fp8_skinny_launches(C, rows_hint, rows_typ, narrow_rows=NARROW_ROWS):
    """k_gemm_skinny_f8 launches of ONE fp8 forward (conv3's and conv4's)."""
    return sum(skinny_launched(layer, "fp8", rows_hint, rows_typ, narrow_rows) for layer in ("conv3", "conv4"))


# ---- the lines ------------------------------------------------------------------------------------------------------
class Line:
    """One hand-over: with (rows_hint, rows_typ) in one of `regimes`, `layer`'s route differs between n = low and n = low + 1.
    A line whose name ends in "shut" is the same pair of n under estimates that keep the second kernel from being launched: one
    kernel takes both sides.  A regime is (hint, typ): hint "n" (rows_hint = n), "pow2" (the next power of two >= n, a captured graph's bound) or a
    number; typ a number (0 = no estimate) or "pow2" (the power of two >= n: a captured graph's pair)."""

    def __init__(self, layer, what, low, regimes, near=True):
        self.layer, self.what, self.low, self.regimes, self.near = layer, what, low, tuple(regimes), near

    def key(self):
        return (self.layer, self.what, self.low)

    def triple(self, n, regime):
        hint, typ = regime
        h = n if hint == "n" else pow2_up(n) if hint == "pow2" else hint
        t = pow2_up(n) if typ == "pow2" else typ
        return (n, max(h, n), t)

    def sides(self):
        """[(regime, low triple, high triple)]"""
        return [(r, self.triple(self.low, r), self.triple(self.low + 1, r)) for r in self.regimes]

    def triples(self):
        out = []
        for r, a, b in self.sides():
            out += [a, b]
        if self.near and self.low > 1:
            out.append(self.triple(self.low - 1, self.regimes[0]))
        return out


def _last_true(pred, hi=MAX_BATCH):
    """All n in [1, hi) with pred(n) != pred(n + 1)."""
    return [n for n in range(1, hi) if pred(n) != pred(n + 1)]


def _tile_lines(layer, C, fam, hi):
    """The n at which `fam`'s tile changes.  The two-per-CU conv family's cost rule moves the tile dozens of times between the same four
    kernels: of those lines, the first of every distinct (tile, next tile) pair and the last one."""
    at = _last_true(lambda k: ring_kernel(layer, C, k, fam), hi)
    if fam != "two" or layer not in ("conv3", "conv4"):
        return at
    seen, keep = set(), []
    for n in at:
        pair = (ring_kernel(layer, C, n, fam), ring_kernel(layer, C, n + 1, fam))
        if pair not in seen or n == at[-1]:
            keep.append(n)
        seen.add(pair)
    return keep


@functools.lru_cache(maxsize=None)
def lines(C, cls, max_batch=MAX_BATCH):
    """Every line of the shipped options at width C, with the regimes in which it is live."""
    MB = max_batch
    out = []
    # skinny hand-overs: the bound itself, the next power of two, and under the largest bound with the estimate at the last value that
    # keeps the small kernel in play, the first that drops it, and none (= the bound: dropped)
    for layer in LAYERS:
        lim = skinny_lim(layer, cls)
        out.append(Line(layer, "skinny hand-over", lim, [("n", 0), ("pow2", 0), (MB, 16 * lim)]))
        out.append(Line(layer, "skinny hand-over shut", lim, [(MB, 16 * lim + 1), (MB, 0)], near=False))
        for n in _last_true(lambda k: skinny_tile(layer, C, k), lim):
            out.append(Line(layer, "skinny 1x1 -> 2x2", n, [("n", 0), (MB, 16 * lim)], near=False))
    if cls == "bf16":
        # conv3's ring (small estimates only): its tile lines, under its three regimes
        small_typ = max(t for t in range(1, 1024) if conv3_is_small(MB, t))
        for n in _last_true(lambda k: ring_kernel("conv3", C, k, "one"), MB):
            regs = ([("n", 0)] if n + 1 <= small_typ else []) + [(MB, small_typ)] + ([("pow2", pow2_up(n) // 2)] if pow2_up(n) // 2 <= small_typ else [])
            out.append(Line("conv3", "ring tile", n, regs, near=False))
        # conv3's tail: the first four lines under every bound, the later ones tight and under the largest bound
        cuts = _last_true(lambda k: conv3_cut(k, C), MB)
        for i, n in enumerate(cuts):
            out.append(Line("conv3", "tail", n, [("n", 0), (MB, 0), ("pow2", 0)] if i < 4 else [(("n", 0), (MB, 0))[i % 2]], near=i < 4))
    else:
        for fam, regs in (("one", [("n", 0)]), ("two", [("n", 0), (MB, 0)])):
            for n in _tile_lines("conv3", C, fam, MB):
                live = [r for r in regs if ring_family("conv3", C, *Line("conv3", "", n, [r]).triple(n, r)[1:]) == fam
                        and ring_family("conv3", C, *Line("conv3", "", n, [r]).triple(n + 1, r)[1:]) == fam]
                if live:
                    out.append(Line("conv3", f"ring tile ({fam})", n, live, near=False))
    # conv4 and the FCs on the ring: the tile lines of each family where that family is what the host picks
    for layer in ("conv4", "fc1", "fc2"):
        m_one = ring_m_one(layer, C) // RPS[layer]
        one_typ = max([t for t in range(1, MB + 1) if ring_family(layer, C, MB, t) == "one"], default=0)
        two_typ = MB
        for fam, regs in (("one", [("n", 0), (MB, one_typ)]), ("two", [("n", 0), (MB, two_typ)])):
            for n in _tile_lines(layer, C, fam, MB):
                live = []
                for r in regs:
                    lo, hi = (Line(layer, "", n, [r]).triple(k, r) for k in (n, n + 1))
                    if r[1] and ring_family(layer, C, lo[1], lo[2]) == fam and ring_family(layer, C, hi[1], hi[2]) == fam:
                        live.append(r)
                    elif not r[1] and route(cls, C, *lo)[layer][1:3] != route(cls, C, *hi)[layer][1:3]:
                        live.append(r)
                if live:
                    if fam == "two" or layer == "fc2":      # large n: one regime each, taken in turn
                        live = [live[len(out) % len(live)]]
                    out.append(Line(layer, f"ring tile ({fam})", n, live, near=False))
        if layer != "conv4" and m_one < MB:
            # the FC window: open at its two ends and on a captured graph's pair; shut just outside either end
            win = [t for t in range(1, MB + 1) if ring_family(layer, C, MB, t) == "window"]
            out.append(Line(layer, "family window", m_one, [(MB, pow2_up(m_one)), (MB, win[0]), (MB, win[-1]), ("n", 0)]))
            out.append(Line(layer, "family window shut", m_one, [(MB, win[0] - 1), (MB, win[-1] + 1)], near=False))
    return out


def host_cases(C, cls, max_batch=MAX_BATCH):
    """Triples on both sides of the lines the HOST draws in (rows_hint, rows_typ) alone, each with a tiny, a middling and a full batch."""
    MB = max_batch
    out = []
    typs = set()
    for layer in LAYERS:
        fams = [ring_family(layer, C, MB, t) for t in range(1, MB + 1)]
        typs |= {t for t in range(1, MB) if fams[t - 1] != fams[t]} | {t + 1 for t in range(1, MB) if fams[t - 1] != fams[t]}
    if cls == "bf16":
        t = max(t for t in range(1, 1024) if conv3_is_small(MB, t))
        typs |= {t, t + 1}
        k = skinny_lim("conv3", cls) + 1          # the smallest batch that is conv3's tiled kernel's
        out += [(t, t, 0), (t + 1, t + 1, 0), (k, t, 0), (k, t + 1, 0), (k, MB, t), (k, MB, t + 1)]
    for t in sorted(typs):
        out += [(1, MB, t), (min(t, MB), MB, t)]
    out.append((MB, MB, min(typs)))           # the one-per-CU families on a full batch: several rounds
    return out


def cases(C, cls, max_batch=MAX_BATCH, only=None):
    return list(_cases(C, cls, max_batch, None if only is None else frozenset(only)))


@functools.lru_cache(maxsize=None)
def _cases(C, cls, max_batch, only):
    """The sorted, distinct (n, rows_hint, rows_typ) triples of width C: both sides of every line (of the lines in `only`, if given)
    plus ALWAYS_N under the tight bound, the next power of two and the largest bound."""
    out = set()
    for ln in lines(C, cls, max_batch):
        if only is None or ln.key() in only:
            out |= set(ln.triples())
    if only is None:
        out |= set(host_cases(C, cls, max_batch))
    for n in ALWAYS_N:
        out |= {(n, n, 0), (n, pow2_up(n), 0), (n, max_batch, 0)}
    assert all(1 <= n <= h <= max_batch and t >= 0 for n, h, t in out)
    # an estimate of 0 or above the bound is the bound (norm_typ): of the triples that are one forward, keep the first
    seen, keep = set(), []
    for n, h, t in sorted(out):
        if (n, h, norm_typ(h, t)) not in seen:
            keep.append((n, h, t))
        seen.add((n, h, norm_typ(h, t)))
    return keep


@functools.lru_cache(maxsize=None)
def moved_lines(C, base=512, cls="bf16"):
    """The keys of width C's lines that width `base` does not have."""
    have = {ln.key() for ln in lines(base, cls)}
    return {ln.key() for ln in lines(C, cls)} - have

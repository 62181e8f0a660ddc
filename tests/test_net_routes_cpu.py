"""Host-only checks of tests/net_routes.py, the restatement of the inference forward's kernel routes that picks the batch sizes of
tests/test_net_routes_gpu.py: (a) the case lists hold both sides of every line under every (rows_hint, rows_typ) regime the line
is live in, (b) the constants the lines rest on are still the ones in the text of csrc/az_net.hip / az_net.h -- whoever moves a
line is sent here to move the cases with it -- and (c) the restated ring_pick_bm agrees with closed forms at the tile changes.
No GPU, no library load."""
import os
import re
from fractions import Fraction

import pytest

import net_routes as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphazero-rs_amd", "csrc")
WIDTHS = [(512, "bf16"), (512, "fp8"), (256, "bf16"), (256, "fp8")]


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _forwards(cases):
    """The forwards a case list runs: the estimate as convnet_forward sees it."""
    return {(n, h, R.norm_typ(h, t)) for n, h, t in cases}


# ---- (a) both sides of every line -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,cls", WIDTHS)
def test_every_line_has_both_sides_in_every_regime(C, cls):
    cases = R.cases(C, cls)
    have = _forwards(cases)
    lines = R.lines(C, cls)
    assert len(cases) == len(set(cases)) == len(have)
    for ln in lines:
        assert ln.regimes, ln.key()
        for regime, lo, hi in ln.sides():
            assert lo[0] + 1 == hi[0] == ln.low + 1
            for n, h, t in (lo, hi):
                assert (n, h, R.norm_typ(h, t)) in have, (ln.key(), regime, (n, h, t))
            a, b = R.route(cls, C, *lo)[ln.layer], R.route(cls, C, *hi)[ln.layer]
            if ln.what.endswith("shut"):                # no hand-over on the device here: one kernel takes both sides
                assert a == b and (a[3] in ("one", "two") if ln.what == "family window shut" else a[-1] is False), (ln.key(), regime, a, b)
            else:
                assert a != b, (ln.key(), regime, a, b)
    # every hand-over kind is present for every layer that has it
    kinds = {(ln.layer, ln.what.split(" (")[0]) for ln in lines}
    assert {(layer, what) for layer in R.LAYERS for what in ("skinny hand-over", "skinny hand-over shut")} <= kinds
    assert ("fc1", "family window") in kinds and ("fc1", "family window shut") in kinds
    assert {("conv4", "ring tile"), ("fc1", "ring tile"), ("fc2", "ring tile"), ("conv3", "ring tile")} <= kinds
    assert (("conv3", "tail") in kinds) == (cls == "bf16")
    for n in R.ALWAYS_N:
        assert {(n, n, n), (n, R.pow2_up(n), R.pow2_up(n)), (n, R.MAX_BATCH, R.MAX_BATCH)} <= have


@pytest.mark.parametrize("C,cls", WIDTHS)
def test_the_host_only_lines_have_both_sides(C, cls):
    """The family choices the host makes from (rows_hint, rows_typ) alone: for each, an estimate on either side under the largest
    bound, with a one-row batch and with a batch of the estimate's size."""
    have = _forwards(R.cases(C, cls))
    MB = R.MAX_BATCH
    for layer in R.LAYERS:
        fams = [R.ring_family(layer, C, MB, t) for t in range(1, MB + 1)]
        for t in range(1, MB):
            if fams[t - 1] != fams[t]:
                for n in (1, t):
                    assert {(n, MB, t), (min(n + 1, t + 1) if n > 1 else 1, MB, t + 1)} <= have, (layer, t)
    if cls == "bf16":
        t = max(t for t in range(1, 1024) if R.conv3_is_small(MB, t))
        for n, h in ((33, MB), (t, MB), (33, None), (t, None)):           # a tiny batch and one of the estimate's size; a far and a tight bound
            lo, hi = (n, h or t, t), (n + (n == t), h or t + 1, t + 1)
            assert (R.route(cls, C, *lo)["conv3"][0], R.route(cls, C, *hi)["conv3"][0]) == ("ring", "image"), (lo, hi)
            assert {lo, hi} <= have, (lo, hi)
    for layer in R.LAYERS:                  # the estimate that keeps / drops the small kernel, on both sides of the hand-over
        lim = R.skinny_lim(layer, cls)
        for n in (lim, lim + 1):
            assert {(n, MB, 16 * lim), (n, MB, 16 * lim + 1)} <= have, (layer, n)
            assert R.skinny_launched(layer, cls, MB, 16 * lim) and not R.skinny_launched(layer, cls, MB, 16 * lim + 1)
            assert R.route(cls, C, lim, MB, 16 * lim)[layer][0] == "skinny" and R.route(cls, C, lim + 1, MB, 16 * lim)[layer][0] != "skinny"


def test_list_sizes():
    """A width's list stays near 150 triples (the GPU sweep runs each under seven option sets); the second width only adds the lines
    that moved."""
    for cls in ("bf16", "fp8"):
        assert 100 <= len(R.cases(512, cls)) <= 180, len(R.cases(512, cls))
        moved = R.moved_lines(256, 512, cls)
        assert moved and len(R.cases(256, cls, only=moved)) <= 80
        assert all(key[0] in ("conv3", "conv4") for key in moved)        # the FCs' widths do not depend on C


def test_the_lines_at_512_channels():
    """The lines as read from the code, by hand, at C = 512 with the shipped options."""
    C = 512
    assert [R.skinny_lim(layer, "bf16") for layer in R.LAYERS] == [32, 64, 128, 128]
    assert [R.skinny_lim(layer, "fp8") for layer in ("conv3", "conv4")] == [32, 64]
    assert R.skinny_launched("conv3", "bf16", 8192, 512) and not R.skinny_launched("conv3", "bf16", 8192, 513)
    assert R.skinny_launched("fc1", "bf16", 2048, 0) and not R.skinny_launched("fc1", "bf16", 2049, 0)
    # conv3's family.  convnet_forward turns "no estimate" into the bound, so the bound gets the 15 % too: 356, not 409
    assert R.conv3_is_small(8192, 356) and not R.conv3_is_small(8192, 357)
    assert R.conv3_is_small(356, 0) and not R.conv3_is_small(357, 0) and not R.conv3_is_small(409, 0)
    assert R.route("bf16", C, 33, 8192, 357)["conv3"][0] == "image" and R.route("bf16", C, 33, 8192, 356)["conv3"][0] == "ring"
    # conv3's tail
    cut = [n for n in range(1, 3073) if R.conv3_cut(n, C)]
    assert cut == list(range(1, 385)) + list(range(1537, 1921))
    assert [n for n in range(1, 8192) if R.conv3_cut(n, C) != R.conv3_cut(n + 1, C)] == [384, 1536, 1920, 3072, 3456, 4608, 4992, 6144, 6528, 7680, 8064]
    assert [n for n in range(1, 8192) if R.conv3_cut(n, 256) != R.conv3_cut(n + 1, 256)] == [768, 3072, 3840, 6144, 6912]
    # the host's grid always holds the tiles the device maps, and every cut tile's second half
    for n, h, _ in R.cases(C, "bf16"):
        assert R.conv3_grid(h, C)[0] >= R.conv3_wid(n, C) and R.conv3_wid(n, C) % 512 <= R.conv3_grid(h, C)[1] or not R.conv3_cut(n, C)
    # the FC family window
    assert R.ring_m_one("fc1", C) == 4096 and R.ring_m_one("fc2", C) == 8192 and R.ring_m_one("conv4", C) == 6144
    win = [t for t in range(1, 8193) if R.ring_family("fc1", C, 8192, t) == "window"]
    assert (win[0], win[-1]) == (2494, 4986) and win == list(range(2494, 4987))
    assert {t * 115 // 100 for t in (2494, 4986)} == {2868, 5733} and 2493 * 115 // 100 < 2868 and 4987 * 115 // 100 > 5734
    assert R.ring_family("fc1", C, 4096, 4096) == "one" and R.ring_family("fc1", C, 4097, 4097) == "window"
    assert not any(R.ring_family("fc2", C, 8192, t) != "one" for t in range(1, 8193))       # fc2's bound never exceeds its m_one
    assert not any(R.ring_family("conv4", C, 8192, t) == "window" for t in range(1, 8193))
    assert R.ring_kernel("fc1", C, 4096, "window") == (4, 128) and R.ring_kernel("fc1", C, 4097, "window") == (2, 96)
    # conv4's family: the bound fits one round, or the estimate + 15 % does
    assert R.ring_family("conv4", C, 1024, 0) == "one" and R.ring_family("conv4", C, 1025, 0) == "two"
    assert R.ring_family("conv4", C, 8192, 891) == "one" and R.ring_family("conv4", C, 8192, 892) == "two"
    # fp8's conv3 is on the ring at every size
    assert R.ring_family("conv3", C, 307, 0) == "one" and R.ring_family("conv3", C, 308, 0) == "two"
    assert R.fp8_skinny_launches(C, 8192, 512) == 2 and R.fp8_skinny_launches(C, 8192, 513) == 1 and R.fp8_skinny_launches(C, 8192, 1025) == 0


# ---- (b) the constants, from the source text ------------------------------------------------------------------------
def test_constants_are_the_sources():
    net, hdr = _text("az_net.hip"), _text("az_net.h")

    def const(name):
        m = re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, net)
        assert m, name
        return int(m.group(1))

    assert const("C3_TAIL") == R.C3_TAIL and const("C3_NB") == R.C3_NB and const("GBN") == R.GBN and const("SK_SMALL_WAVES") == R.SK_SMALL_WAVES
    assert int(re.search(r"int narrow_rows = (\d+);", hdr).group(1)) == R.NARROW_ROWS
    assert re.search(r"int conv3_small = 1;", hdr) and re.search(r"int conv3_tail = 1;", hdr)
    # conv3_is_small: (estimate * 115 / 100, or the bound) * rows_per_sample <= 8192
    body = re.search(r"static bool conv3_is_small\([^)]*\) \{\s*return ([^\n]*)\n", net).group(1)
    assert "rows_typ * %d / %d" % (R.EST_NUM, R.EST_DEN) in body and body.rstrip().split("//")[0].rstrip().endswith("<= %d;" % R.CONV3_SMALL_ROWS)
    # the clamp of the estimate
    assert "if (rows_typ <= 0 || rows_typ > rows_hint) rows_typ = rows_hint;" in net
    # launch_ring_auto: the estimate, m_one, the window, the grid's smallest tile
    ring = net[net.index("static void launch_ring_auto("):net.index("#ifdef AZ_DIAG", net.index("static void launch_ring_auto("))]
    assert "rows_typ * %d / %d" % (R.EST_NUM, R.EST_DEN) in ring
    assert "const int tile_max = conv ? 96 : 128;" in ring and "const int m_one = 256 / ncol * tile_max;" in ring
    assert "m_one * %d" % R.WINDOW_LO in ring and "m_one * %d" % R.WINDOW_HI in ring and "!conv && m_bound > m_one" in ring
    assert "const int bmin = one_per_cu ? 64 : 96;" in ring
    assert "lo.m_hi = m_one;" in ring and "hi.m_min = std::max(d.m_min, m_one);" in ring
    assert "(m_est + tile_max - 1) / tile_max * ncol <= 256" in ring
    # the skinny rule, bf16 and fp8
    assert net.count("if (est <= %d * lim) {" % R.SKINNY_EST_FACTOR) == 2
    assert net.count("if (rows_hint <= lim) return;") == 2 and net.count("dd.m_max = lim * d.rows_per_sample;") == 2 and net.count("dd.m_min = dd.m_max;") == 2
    m = R.SKINNY_MULT
    assert "o.narrow_rows * (LAYER == 2 ? %d : LAYER == 3 ? %d : %d);" % (m["conv3"], m["conv4"], m["fc1"]) in net and m["fc1"] == m["fc2"]
    assert "o.narrow_rows * (LAYER == 2 ? %d : %d);" % (m["conv3"], m["conv4"]) in net
    assert "if ((M + 15) / 16 * (d.N / 16) <= SK_SMALL_WAVES) {" in net
    # the device side of the hand-overs
    assert "if (M > d.m_max || M <= 0) return;" in net
    assert "if (M <= d.m_min || (d.m_hi > 0 && M > d.m_hi)) return;" in net
    assert "if (n_boards * d.rows_per_sample <= d.m_min) return;" in net
    assert "const bool cut = rem > 0 && rem <= tail_wgs;" in net and "const int full_rounds = wid / 512 * 512, rem = wid - full_rounds;" in net
    assert "const int tiles8 = ((n_boards + C3_NB - 1) / C3_NB + 7) / 8 * 8;" in net
    # ring_pick_bm
    pick = net[net.index("AZ_HD int ring_pick_bm("):net.index("template <int LAYER, int NS>", net.index("AZ_HD int ring_pick_bm("))]
    assert "if (ns == 4) return wgs(64) <= 256 ? 64 : wgs(96) <= 256 ? 96 : 128;" in pick
    assert "if (!conv) return wgs(96) <= 512 ? 96 : 128;" in pick
    assert "for (int bm = 96; bm <= 192; bm += 32) {" in pick
    assert "(10.f + 0.42f * (float)bm) * ((float)full + (rem == 0 ? 0.f : rem <= 256 ? 0.6f : 1.f));" in pick
    # rows per board and widths of the four layers, as convnet_forward sets them
    assert "d.rows_per_sample = 20;" in net and "d.rows_per_sample = 6;" in net and "d.K = 6 * C; d.N = 1024;" in net and "d.K = 1024; d.N = 512;" in net


# ---- (c) ring_pick_bm against closed forms --------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [2, 4, 8])
def test_ring_pick_bm_at_its_tile_changes(ncol):
    top = 8192 * 20
    one = [M for M in range(1, top) if R.ring_pick_bm(M, ncol, 4, False) != R.ring_pick_bm(M + 1, ncol, 4, False)]
    assert one == [64 * (256 // ncol), 96 * (256 // ncol)]            # the last M whose 64- / 96-row tiles fit one round of 256
    assert [R.ring_pick_bm(M, ncol, 4, True) for M in (one[0], one[0] + 1, one[1], one[1] + 1)] == [64, 96, 96, 128]
    fc = [M for M in range(1, top) if R.ring_pick_bm(M, ncol, 2, False) != R.ring_pick_bm(M + 1, ncol, 2, False)]
    assert fc == [96 * (512 // ncol)] and R.ring_pick_bm(fc[0], ncol, 2, False) == 96 and R.ring_pick_bm(fc[0] + 1, ncol, 2, False) == 128
    if ncol == 8:
        return
    # the cost rule in exact rationals picks the same tile as the f32 evaluation at every M up to the largest batch: no tile
    # change rests on a rounding (so the restatement's changes are the device's), and the list claims exactly these changes
    def exact(M):
        best, best_cost = 128, None
        for bm in range(96, 193, 32):
            w = (M + bm - 1) // bm * ncol
            full, rem = divmod(w, 512)
            cost = (10 + Fraction(42, 100) * bm) * (full + (0 if rem == 0 else Fraction(6, 10) if rem <= 256 else 1))
            if best_cost is None or cost < best_cost:
                best, best_cost = bm, cost
        return best
    C = ncol * 128
    for layer in ("conv3", "conv4"):
        rps = R.RPS[layer]
        picks = [R.ring_pick_bm(n * rps, ncol, 2, True) for n in range(1, 8194)]
        assert picks == [exact(n * rps) for n in range(1, 8194)]
        assert set(picks) <= {96, 128, 160, 192}
        changes = [n for n in range(1, 8192) if picks[n - 1] != picks[n]]
        kept = [ln.low for ln in R.lines(C, "fp8") if ln.layer == layer and ln.what == "ring tile (two)"]
        assert set(kept) <= set(changes) and kept
        pairs = {(picks[n - 1], picks[n]) for n in changes if R.ring_family(layer, C, n + 1, 0) == "two"}
        assert pairs == {(picks[n - 1], picks[n]) for n in kept}, (layer, pairs)

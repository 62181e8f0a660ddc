"""The step plan of NNet::train (csrc/az_train_plan.h) without a GPU.

  * its g++ build (tests/train_plan_twin.py) against `restate` below, a numpy restatement of the routing rules written from their prose
    statement ("the step plan"), not from the header: every batch 2 .. 256, C in {128, 256, 384, 512}, all 128 switch
    combinations, the side stream present and absent, every field equal; six anchor rows as literals;
  * the case tables of the GPU tests as data: what tests/test_train_shapes_gpu.py (SWEEP_512, SWEEP_512_F32, OTHER_WIDTHS) and
    tests/train_layers_ref.py (TABLE_ROUTES) say a case takes is what the plan gives it;
  * closed-world coverage: every per-layer route fact that some accepted (b, C, switches) reaches is reached by a case the GPU tests run;
  * train_layers_ref.gemm_format (which picks each GEMM's error bound) agrees with the plan on every GEMM of every TABLE_CASES entry;
  * splitk_pick's properties over every GEMM of every plan of the sweep, with the trainer's two workspace sizes;
  * the header compiled alone by g++ with AddressSanitizer and UBSan, run as a stand-alone program (tests/cpp/train_plan_check.cpp).
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import test_train_gpu as TG
import test_train_shapes_gpu as TS
import train_layers_ref as R
import train_plan_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (128, 256, 384, 512)
# trainer_create (csrc/az_train.hip): splitk_floats = 96 << 20 for the caller's stream, splitk2_floats = 16 << 20 for the side branch
WS_MAIN, WS_SIDE = 96 << 20, 16 << 20


def sweep_rows(Cw):
    """Every (switches, side, b) at width Cw as the twin's rows: 128 x 2 x 255 of them."""
    combos = np.array(list(itertools.product((0, 1), repeat=8)), np.int32)            # seven switches, then the side stream
    bs = np.arange(2, 257, dtype=np.int32)
    rows = np.zeros((len(combos), len(bs), 10), np.int32)
    rows[:, :, :8] = combos[:, None, :]
    rows[:, :, 8] = bs[None, :]
    rows[:, :, 9] = Cw
    return rows.reshape(-1, 10)


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------

def restate(rows):
    """rows [n][10] (train_plan_twin.rows_of) -> [n][INTS] int32, from the rules as DESIGN.md states them."""
    rows = np.asarray(rows, np.int64)
    gemm, dma, fwd_x3, wgrad_tr, implicit, ring, fork_sw, side, b, Cw = (rows[:, i] for i in range(10))
    one = np.ones_like(b)
    M = [42 * b, 42 * b, 20 * b, 6 * b, b, b]
    K = [18 * one, 9 * Cw, 9 * Cw, 9 * Cw, 6 * Cw, 1024 * one]
    N = [Cw, Cw, Cw, Cw, 1024 * one, 512 * one]
    LDA = [20 * one, 9 * Cw, 9 * Cw, 9 * Cw, 6 * Cw, 1024 * one]
    out = np.zeros((len(rows), T.INTS), np.int32)
    kern = {k: i for i, k in enumerate(T.KERNEL)}
    up = lambda x, m: (x + m - 1) // m

    x3 = gemm == 1
    fx3 = x3 & (fwd_x3 == 1)
    gathered = fx3 & (implicit == 1) & (wgrad_tr == 1) & (b % 16 == 0) & (20 * b > 64) & (Cw % 256 == 0)
    fork = x3 & (fork_sw == 1) & (side == 1)
    tr = lambda l, rows_: x3 & (wgrad_tr == 1) & (rows_ % 32 == 0) & (K[l] % 256 == 0) & (N[l] % 128 == 0)
    col_tr = lambda l: tr(l, M[l]) if 1 <= l <= 3 else np.zeros_like(x3)
    fc_tr = lambda l: tr(l, b) if l >= 4 else np.zeros_like(x3)

    def put(name, val, l=None, gemm_=None, where=None):
        val = np.broadcast_to(np.asarray(val, np.int64), b.shape)
        c = T.col(name, l, gemm_)
        out[:, c] = val if where is None else np.where(where, val, out[:, c])

    def put_gemm(l, which, kernel, m, n, k, where, side_ws=0):
        for name, v in (("kernel", kernel), ("M", m), ("N", n), ("K", k), ("side_ws", side_ws)):
            put(name, v, l, which, where)

    def f32_kernel(m, n, k, on_dma=None):
        big = (k >= 256) & (up(m, 128) * up(n, 128) >= 64)
        kk = np.where(big, kern["gemm_f32_128"], kern["gemm_f32_64"])
        return kk if on_dma is None else np.where(on_dma, kern["gemm_f32_dma"], kk)

    def x3_kernel(m, kc, gathered_a=False):
        padded = up(m, 256) * 256
        on_ring = (ring == 1) & (kc // 32 >= 16) & ((padded - m) * 10 <= padded)
        return np.where(on_ring | gathered_a, kern["gemm3_ring"], kern["gemm3"])

    put("x3", x3); put("fork", fork); put("perm_conv2", gathered)
    put("split", np.select([~x3, fork, fx3], [T.SPLIT.index("none"), T.SPLIT.index("side_start"), T.SPLIT.index("in_prep")], T.SPLIT.index("after_heads")))
    put("prep", np.select([~fx3, fork], [T.PREP.index("none"), T.PREP.index("two")], T.PREP.index("one")))
    for l in range(6):
        conv234 = 1 <= l <= 3
        # forward
        g_fwd = gathered if conv234 else np.zeros_like(x3)
        c_fwd = (fx3 & ~gathered) if conv234 else np.zeros_like(x3)
        f_fwd = ~g_fwd & ~c_fwd
        put("fwd", np.select([g_fwd, c_fwd], [T.FWD.index("x3_gather"), T.FWD.index("x3_col")], T.FWD.index("f32")), l)
        dma_ok = (dma == 1) & (M[l] >= 128) & (K[l] % 16 == 0) & (K[l] >= 128) & (N[l] % 128 == 0) & (LDA[l] % 4 == 0)
        put_gemm(l, "fwd_gemm", np.where(f_fwd, f32_kernel(M[l], N[l], K[l], dma_ok), x3_kernel(M[l], K[l], g_fwd)), M[l], N[l], K[l], True)
        # BatchNorm
        put("bn_small", M[l] <= 64, l)
        extra = np.zeros_like(b)
        if l <= 2:
            extra = extra | np.where(gathered, 3, 0)
        if l in (3, 4):
            extra = extra | np.where(fc_tr(l + 1), 2, 0)
        put("bn_extra", extra, l)
        if l <= 2:
            ct = col_tr(l + 1)
            put("im2col", np.where(gathered, 0, np.where(fx3, 2, 0) | np.where(ct, 4, 0) | np.where(~fx3 | ~ct, 1, 0)), l)
        # wgrad
        w_f32 = ~x3 if l >= 1 else np.ones_like(x3)
        w_gather = ~w_f32 & g_fwd
        w_act = ~w_f32 & ~w_gather & fc_tr(l)
        w_col = ~w_f32 & ~w_gather & ~w_act & col_tr(l)
        w_tp = ~w_f32 & ~w_gather & ~w_act & ~w_col
        put("wgrad", np.select([w_f32, w_gather, w_act, w_col], [T.WGRAD.index(k) for k in ("f32", "tr_gather", "tr_act", "tr_col")], T.WGRAD.index("transpose")), l)
        put_gemm(l, "wgrad_gemm", f32_kernel(K[l], N[l], M[l]), K[l], N[l], M[l], w_f32)
        put_gemm(l, "wgrad_gemm", kern["wgrad3_tr"], K[l], N[l], M[l], w_gather | w_act | w_col, fork)
        mp = up(M[l], 64) * 64
        put_gemm(l, "wgrad_gemm", x3_kernel(K[l], mp), K[l], N[l], mp, w_tp, fork)
        # dgrad
        if l == 0:
            continue
        d_gather = x3 & gathered if l == 1 else np.zeros_like(x3)
        d_x3 = x3 & ~d_gather
        put("dgrad", np.select([~x3, d_gather], [T.DGRAD.index("f32"), T.DGRAD.index("x3_gather")], T.DGRAD.index("x3")), l)
        put("dgrad_dst", np.where(d_gather | (l >= 4), T.DST.index("dact"), T.DST.index("dcol")), l)
        put_gemm(l, "dgrad_gemm", f32_kernel(M[l], K[l], N[l]), M[l], K[l], N[l], ~x3)
        put_gemm(l, "dgrad_gemm", x3_kernel(M[l], N[l]), M[l], K[l], N[l], d_x3)
        put_gemm(l, "dgrad_gemm", kern["gemm3_ring"], 42 * b, Cw, 9 * N[l], d_gather)
        put("col2im", ~d_gather if conv234 else np.zeros_like(x3), l)
    return out


@pytest.fixture(scope="module")
def sweep():
    """{C: (rows, the header's plans)} over the whole accepted range, computed once."""
    out = {}
    for Cw in WIDTHS:
        rows = sweep_rows(Cw)
        plans = T.plans(rows)
        for a in (rows, plans):
            a.setflags(write=False)
        out[Cw] = (rows, plans)
    return out


@pytest.mark.parametrize("Cw", WIDTHS)
def test_plan_is_the_restated_rules(sweep, Cw):
    rows, plans = sweep[Cw]
    assert len(rows) == 128 * 2 * 255
    want = restate(rows)
    bad = np.argwhere(plans != want)
    assert len(bad) == 0, (rows[bad[0][0]].tolist(), int(bad[0][1]), int(plans[tuple(bad[0])]), int(want[tuple(bad[0])]))


def holds(plan, spec):
    """A case's stated routes against a decoded plan -> the list of disagreements.  spec: {"gathered": bool} and / or {layer field:
    {layer: value}} with the field names of train_plan_twin.decode ("fwd", "wgrad", "dgrad", "bn", "col2im", "im2col", "*_kernel")."""
    bad = []
    for key, val in spec.items():
        if key == "gathered":
            got = plan["perm_conv2"] and all(plan["layers"][l]["fwd"] == "x3_gather" for l in (1, 2, 3))
            none = not plan["perm_conv2"] and all(plan["layers"][l]["fwd"] != "x3_gather" for l in (1, 2, 3))
            if not (got if val else none):
                bad.append((key, val))
        else:
            bad += [(key, l, v, plan["layers"][l][key]) for l, v in val.items() if plan["layers"][l][key] != v]
    return bad


ALL_TRANSPOSE = {l: "transpose" for l in range(1, 6)}
ANCHORS = [
    (512, 2, {}, {"gathered": False, "fwd": {1: "x3_col", 2: "x3_col", 3: "x3_col"}, "wgrad": ALL_TRANSPOSE,
                  "dgrad": {l: "x3" for l in range(1, 6)}, "col2im": {1: True, 2: True, 3: True},
                  "bn": {0: "large", 1: "large", 2: "small", 3: "small", 4: "small", 5: "small"}}),
    (512, 8, {}, {"gathered": False, "wgrad": {1: "transpose", 2: "tr_col", 3: "transpose"}}),
    (512, 16, {}, {"gathered": True, "wgrad": {1: "tr_gather", 2: "tr_gather", 3: "tr_gather", 4: "transpose", 5: "transpose"},
                   "dgrad": {1: "x3_gather"}, "col2im": {1: False}}),
    (512, 64, {}, {"gathered": True, "wgrad": {4: "tr_act", 5: "tr_act"}, "bn": {3: "large", 4: "small", 5: "small"}}),
    (512, 37, {}, {"gathered": False, "wgrad": ALL_TRANSPOSE}),
    (384, 64, {}, {"gathered": False, "wgrad": {1: "transpose", 2: "transpose", 3: "transpose", 4: "tr_act", 5: "tr_act"}}),
]


@pytest.mark.parametrize("Cw,b,sw,spec", ANCHORS, ids=[f"C{a[0]}-b{a[1]}" for a in ANCHORS])
def test_anchor_rows(Cw, b, sw, spec):
    assert holds(T.plan(Cw, b, sw), spec) == []


def test_defaults_are_the_shipped_defaults():
    assert np.array_equal(T.rows_of([(512, 64, {}, False)])[0, :7], [1, 1, 1, 1, 1, 1, 0])
    src = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_train_plan.h")).read()
    for key, val in T.DEFAULTS.items():
        assert f"int {key[len('train_'):]} = {val};" in src, key


# ---- the GPU tests' case tables ------------------------------------------------------------------------------------------------------

def set_switches(gemm_set):
    return dict(zip(("train_gemm", "train_fwd_dma", "train_fwd_x3"), gemm_set))


def stated_cases():
    """(what, C, b, switches, spec) of every GPU case that states its routes."""
    out = [(f"SWEEP_512[{b}]", 512, b, {}, spec) for b, spec in TS.SWEEP_512.items()]
    out += [(f"SWEEP_512_F32[{b}]", 512, b, {"train_gemm": 0}, spec) for b, spec in TS.SWEEP_512_F32.items()]
    out += [(f"OTHER_WIDTHS[{Cw}, {b}]", Cw, b, {}, spec) for (Cw, b), spec in TS.OTHER_WIDTHS.items()]
    out += [(f"NEW_ROUTES[{Cw}, {b}]", Cw, b, sw, spec) for Cw, b, sw, spec in TS.NEW_ROUTES]
    for case in R.TABLE_CASES:
        Cw, gs, sw, b = case
        out.append((R.case_id(case), Cw, b, {**set_switches(gs), **sw}, R.TABLE_ROUTES[R.case_id(case)]))
    return out


def test_every_table_case_states_its_routes():
    assert set(R.TABLE_ROUTES) == {R.case_id(c) for c in R.TABLE_CASES}
    assert all(spec for _, _, _, _, spec in stated_cases())


@pytest.mark.parametrize("what,Cw,b,sw,spec", stated_cases(), ids=[c[0] for c in stated_cases()])
def test_stated_routes_are_the_plans(what, Cw, b, sw, spec):
    assert holds(T.plan(Cw, b, sw), spec) == [], what


# ---- closed-world coverage -------------------------------------------------------------------------------------------------------------

def gpu_cases():
    """(C, b, switches, side stream exists) of the steps tests/test_train_shapes_gpu.py, tests/test_train_layers_gpu.py and
    tests/test_train_gpu.py take on the GPU (not all of them: the ones listed here are enough, and each is read off those modules)."""
    cases = [(Cw, b, sw, False) for _, Cw, b, sw, _ in stated_cases()]
    # test_dropout_on_the_large_row_kernels_c128: the e128 fixture runs every GEMM set
    cases += [(128, b, set_switches(gs), False) for gs in TG.GEMM_SETS for b in TS.DROPOUT_C128]
    # test_shipped_switches_off_at_c512, test_fork_is_bit_identical_at_c512 (the fork creates the side stream)
    cases += [(512, b, {sw: 0}, False) for sw in TS.SHIPPED_SWITCHES for b in TS.SWITCH_BATCHES]
    cases += [(512, b, {"train_fork": 1}, True) for b in TS.SWITCH_BATCHES]
    # test_az_net_train_is_the_documented_sequence_of_steps: batch 32 at C = 128 in every GEMM set, with the fork as well
    cases += [(TG.C, 32, {**set_switches(gs), "train_fork": f}, bool(f)) for gs in TG.GEMM_SETS for f in (0, 1)]
    # test_f16x3_forward_range: b = 64 in the default and the f32 set
    cases += [(512, 64, {}, False), (512, 64, {"train_gemm": 0}, False)]
    return cases


def facts(plans):
    """The per-layer route facts of plans [n][INTS] -> a set of tuples."""
    out = set()
    out |= {("prep",T.SPLIT[s], T.PREP[p]) for s, p in np.unique(plans[:, [T.col("split"), T.col("prep")]], axis=0)}
    for l in range(6):
        pick = lambda *cols: np.unique(plans[:, list(cols)], axis=0)
        out |= {("fwd", l, T.FWD[r], T.KERNEL[k]) for r, k in pick(T.col("fwd", l), T.col("kernel", l, "fwd_gemm"))}
        out |= {("wgrad", l, T.WGRAD[r]) for r, in pick(T.col("wgrad", l))}
        out |= {("dgrad", l, T.DGRAD[r]) for r, in pick(T.col("dgrad", l))}
        out |= {("bn", l, "small" if s else "large") for s, in pick(T.col("bn_small", l))}
        out |= {("im2col", l, tuple(sorted(T._set(int(m), T.COL)))) for m, in pick(T.col("im2col", l))}
    return out


def test_every_reachable_route_runs_on_the_gpu(sweep):
    universe = set()
    for Cw in WIDTHS:
        universe |= facts(sweep[Cw][1])
    reached = facts(T.plans(T.rows_of(gpu_cases())))
    assert reached <= universe
    assert sorted(universe - reached) == []


# ---- the per-kernel tests' bound selection -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.TABLE_CASES, ids=R.case_id)
def test_gemm_format_agrees_with_the_plan(case):
    Cw, gs, sw, b = case
    plan = T.plan(Cw, b, {**set_switches(gs), **sw})
    for l, lp in enumerate(plan["layers"]):
        assert R.gemm_format("fwd", l, gs) == ("f16x3" if lp["fwd"] in ("x3_gather", "x3_col") else "f32"), l
        assert R.gemm_format("wgrad", l, gs) == ("f32" if lp["wgrad"] == "f32" else "bf16x3"), l
        if l >= 1:
            assert R.gemm_format("dgrad", l, gs) == ("f32" if lp["dgrad"] == "f32" else "bf16x3"), l


# ---- split-K -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cw", WIDTHS)
def test_splitk_of_every_gemm_of_every_plan(sweep, Cw):
    plans = sweep[Cw][1]
    first = T.col("kernel", 0, "fwd_gemm")
    gemms = np.concatenate([plans[:, T.col("kernel", l, g):T.col("kernel", l, g) + 5] for l in range(6) for g in T.GEMMS])
    assert first == len(T.STEP_FIELDS) + len(T.LAYER_FIELDS)
    gemms = np.unique(gemms[gemms[:, 0] != 0], axis=0)
    assert len(gemms) > 1000
    steps, want, sps, splits = (c.astype(np.int64) for c in T.gemm_splits(gemms, WS_MAIN, WS_SIDE).T)
    out_elems = gemms[:, 1].astype(np.int64) * gemms[:, 2]
    ws = np.where(gemms[:, 4] == 1, WS_SIDE, WS_MAIN)
    assert (steps >= 1).all() and (splits >= 1).all()
    assert ((splits * out_elems <= ws) | (splits == 1)).all()
    assert (splits * sps >= steps).all()
    assert ((splits - 1) * sps < steps).all()                       # no slice is empty
    assert (splits[want <= 1] == 1).all() and (splits <= np.maximum(want, 1)).all()
    # the picker alone on the same arguments, and with a workspace that holds two slices only
    again = T.splitk_pick(np.stack([steps, want, out_elems, ws], axis=1))
    assert np.array_equal(again[:, 0], sps) and np.array_equal(again[:, 1], splits)
    tight = T.splitk_pick(np.stack([steps, want, out_elems, 2 * out_elems], axis=1)).astype(np.int64)
    assert (tight[:, 1] <= 2).all() and (tight[:, 1] * tight[:, 0] >= steps).all() and ((tight[:, 1] - 1) * tight[:, 0] < steps).all()


# ---- the header alone --------------------------------------------------------------------------------------------------------------------

def test_header_alone_under_sanitizers(tmp_path):
    """csrc/az_train_plan.h needs nothing of HIP: g++ compiles it alone, and the stand-alone program walks the whole sweep clean under
    ASan + UBSan."""
    exe = os.path.join(tmp_path, "train_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "alphazero-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "train_plan_check.cpp"), "-o", exe])
    assert subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip() == "ok"

"""The plan the engine's trainer follows (the diagnostic library's az_diag_train_plan: csrc/az_train_plan.h as az_set_option and
az_net_train_begin hand it the switches) against the g++ twin of the same header under the same switches.  Every route of a step computes
a correct gradient, so no numerical test can see a switch wired to the wrong field; this one does.  Host only: nothing is launched beyond
az_net_train_begin's uploads."""
import ctypes

import numpy as np
import pytest

import train_plan_twin as T

pytestmark = pytest.mark.gpu

BATCHES = (2, 16, 32, 37, 64)
COMBOS = [{}] + [{k: 1 - v} for k, v in T.DEFAULTS.items()] + [{"train_gemm": 0, "train_fwd_dma": 0}]


def engine_plan(e, b):
    f = e._lib.az_diag_train_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    out = np.full(T.INTS, -7, np.int32)
    assert f(e._h, b, out.ctypes.data_as(ctypes.c_void_p), T.INTS) == T.INTS, b
    return out


def test_engine_plan_is_the_twins_under_every_switch(engine_mod):
    assert not hasattr(engine_mod._lib, "az_diag_train_plan")              # the diagnostic library only
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=256, diag=True)
    try:
        f = e._lib.az_diag_train_plan
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        buf = np.zeros(T.INTS, np.int32)
        assert f(e._h, 64, buf.ctypes.data_as(ctypes.c_void_p), T.INTS) == -1, "no training session yet"
        e.net_init_random(1, seed=1)
        e.set_option("train_implicit", 0)                                   # set before the trainer exists: az_net_train_begin forwards the record
        e.train_begin(1)
        assert np.array_equal(engine_plan(e, 32), T.plans(T.rows_of([(256, 32, {"train_implicit": 0}, False)]))[0])
        e.set_option("train_implicit", 1)
        for b, cap in ((1, T.INTS), (257, T.INTS), (64, T.INTS - 1)):
            assert f(e._h, b, buf.ctypes.data_as(ctypes.c_void_p), cap) == -1, (b, cap)
        for combo in COMBOS:
            try:
                for key, val in combo.items():
                    e.set_option(key, val)
                # "train_fork" 1 creates the side stream; while the switch is 0 the plan does not ask whether one exists
                want = T.plans(T.rows_of([(256, b, combo, combo.get("train_fork") == 1) for b in BATCHES]))
                for b, w in zip(BATCHES, want):
                    got = engine_plan(e, b)
                    bad = np.nonzero(got != w)[0]
                    assert len(bad) == 0, (combo, b, bad.tolist(), got[bad].tolist(), w[bad].tolist())
            finally:
                for key, val in T.DEFAULTS.items():
                    e.set_option(key, val)
        assert np.array_equal(engine_plan(e, 64), T.plans(T.rows_of([(256, 64, {}, False)]))[0])
        e.train_end(2)
    finally:
        e.close()

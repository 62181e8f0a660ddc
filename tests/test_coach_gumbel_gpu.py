"""The two Coaches with Gumbel root search on (Coach.gumbel_m / gumbel_c_visit / gumbel_c_scale in coach.py and include/az_host.hpp): one
iteration of tests/test_coach_gpu.py::test_python_and_cpp_coach_agree in miniature on both hosts -- same report, byte-identical files --, the
option on for the episodes only and off again before the arena."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg        # noqa: E402

M, C_VISIT, C_SCALE, SIMS = 4, 12.5, 2.0, 16
KEYS = ("gumbel_c_visit_e6", "gumbel_c_scale_e6", "gumbel_m")


def run_python(engine_mod, d, gumbel, seen=None):
    from alphazero_rs_amd.coach import Coach
    e = engine_mod.Engine(device=0, max_batch=256, net_channels=128)
    try:
        e.net_init_random(0, 3)
        e.set_option("train_epochs", 1)
        coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, SIMS, 1, 1000, 1, log=lambda m: None)
        if gumbel:
            coach.gumbel_m, coach.gumbel_c_visit, coach.gumbel_c_scale = M, C_VISIT, C_SCALE
            coach.root_noise_eps, coach.root_noise_alpha = 0.25, 0.3
        if seen is not None:
            orig_set, orig_arena = e.set_option, e.arena

            def spy(key, value):
                if key in KEYS:
                    seen.append((key, value))
                return orig_set(key, value)

            def arena_spy(*a, **kw):
                seen.append(("arena", 0))
                return orig_arena(*a, **kw)
            e.set_option, e.arena = spy, arena_spy
        return coach.learn(seed=11)
    finally:
        e.close()


def test_python_and_cpp_coach_agree_with_gumbel(engine_mod, tmp_path):
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}
    seen = []
    rep = run_python(engine_mod, dirs["py"], True, seen)
    run_python(engine_mod, dirs["plain"], False)
    exe = os.path.join(tmp_path, "test_coach_gumbel")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_gumbel.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], "128", "11", f"gumbel_m={M}", f"gumbel_c_visit={C_VISIT}", f"gumbel_c_scale={C_SCALE}",
                          "root_noise_eps=0.25", "root_noise_alpha=0.3", f"num_sims={SIMS}"], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == 1
    for k in fg.REPORT_KEYS:
        assert rep[0][k] == crep[0][k], k
    fg.compare_directories(dirs["py"], dirs["cpp"])
    with open(os.path.join(dirs["py"], "0.examples"), "rb") as x, open(os.path.join(dirs["plain"], "0.examples"), "rb") as y:
        assert x.read() != y.read()                                  # the option really shaped the episodes
    # on for the episodes, off again behind them -- before the arena
    assert seen == [("gumbel_c_visit_e6", 12500000), ("gumbel_c_scale_e6", 2000000), ("gumbel_m", M),
                    ("gumbel_c_visit_e6", 50000000), ("gumbel_c_scale_e6", 1000000), ("gumbel_m", 0), ("arena", 0)], seen

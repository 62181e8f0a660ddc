"""The shared tree batch without a GPU: its request combiner (alphazero-rs_amd/csrc/az_combine.h, no HIP in it) built with
-fsanitize=thread and driven by 64 threads through a fake batch runner, and the new C++ host code compiled and linked against
the library."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero-rs_amd", "csrc")


@pytest.fixture(scope="module")
def combiner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("combine") / "test_combine_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_combine_cpu.cpp"), "-o", exe])
    return exe


def run(exe, *args):
    # TSan reports go to stderr and make the exit status non-zero (halt_on_error keeps a report from being lost in the noise);
    # the binary's own watchdog exits non-zero on a deadlock before this limit
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr[-4000:])
    assert "ThreadSanitizer" not in p.stderr, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("slots,window_us", [(48, 0), (64, 0), (48, 100), (64, 50)])
def test_combiner_random_threads(combiner, slots, window_us):
    """64 threads acquire, submit, release and re-acquire slots at random: every request is answered exactly once with its own
    result, no batch holds a slot twice, one leader at a time, and with window 0 a batch starts only when every held slot waits."""
    got = run(combiner, "random", 64, slots, 200, window_us)
    assert got["wrong"] == 0 and got["refused"] == 0, got
    assert got["submitted"] == got["requests"] == got["stats"][1], got
    assert got["batches"] == got["stats"][0], got
    assert got["dup_slot"] == 0 and got["runner_overlap"] == 0, got
    assert got["not_full"] == 0, got
    assert got["stats"][2] <= slots
    if window_us == 0:
        assert got["by_window"] == 0 and got["stats"][3] == 0
    if slots == 64:
        assert got["capacity"] == 0           # 64 slots for 64 threads: an acquire never fails
    assert got["requests"] > got["batches"]  # requests were coalesced


def test_window_starts_batches_when_a_thread_stalls(combiner):
    got = run(combiner, "stall", 1000)
    assert got["wrong"] == 0 and got["dup_slot"] == 0
    assert got["done_before_stall_end"] == 3      # the three busy threads finished while the fourth slot's thread stalled
    assert got["by_window"] >= 20


def test_window_zero_waits_for_every_held_slot(combiner):
    got = run(combiner, "stall", 0)
    assert got["wrong"] == 0 and got["not_full"] == 0
    assert got["done_after"] == 3 and got["by_window"] == 0


def test_release_wakes_the_waiters(combiner):
    got = run(combiner, "release")
    assert got["wrong"] == 0 and got["not_full"] == 0
    assert got["done_after"] == 3                  # they could only go on once the holder let its slot go


@pytest.mark.parametrize("src", [os.path.join("tests", "cpp", "test_shared_tree.cpp"), os.path.join("examples", "concurrent_dropin.cpp")])
def test_shared_tree_programs_compile_and_link(engine_mod, src, tmp_path):
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    exe = os.path.join(tmp_path, "prog")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, src), "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    assert os.path.exists(exe)


def test_python_binding_declares_the_shared_tree(engine_mod):
    for name in ("az_tree_share", "az_tree_slot_acquire", "az_tree_slot_release", "az_tree_slot_get_action_prob",
                 "az_tree_slot_error", "az_tree_share_stats"):
        assert name in engine_mod.EXPORTS
    for meth in ("share", "slot_acquire", "slot_release", "slot_get_action_prob", "share_stats"):
        assert callable(getattr(engine_mod.TreeBatch, meth))

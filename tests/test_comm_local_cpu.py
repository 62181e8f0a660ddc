"""The in-process communicator (az_comm_local_id) without a GPU: its rendezvous (alphazero-rs_amd/csrc/az_local_comm.h, no HIP in it)
built with -fsanitize=thread and driven by 2..8 threads through many rounds of random collectives on host data, plus the new C++
host code compiled and linked against the library and the binding's declaration of the new export."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alphazero-rs_amd", "csrc")


@pytest.fixture(scope="module")
def rendezvous(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("local_comm") / "test_local_comm_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_local_comm_cpu.cpp"), "-o", exe])
    return exe


def run(exe, *args):
    # TSan reports go to stderr and make the exit status non-zero; the binary's own watchdog exits non-zero on a deadlock first
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr[-4000:])
    assert "ThreadSanitizer" not in p.stderr, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("world,seed", [(2, 1), (3, 2), (4, 3), (5, 4), (8, 5)])
def test_random_collectives(rendezvous, world, seed):
    """Every rank runs the same seeded sequence of 400 collectives (gathers of ragged counts with dst 0..world-1 or -1, sums of n =
    0..64 u64 that wrap, 3-counter sums) with random delays; about one round in eight one rank calls another collective or passes
    another n / dst_rank.  Correct rounds return exactly the rank-order concatenation / the sum; mismatched ones fail on every rank
    with the same message, and the next round works."""
    got = run(rendezvous, "random", world, 400, seed)
    assert got["rounds"] == 400 * world
    assert got["wrong"] == 0 and got["errors_unexpected"] == 0 and got["missing_error"] == 0, got
    assert got["message_differs"] == 0, got
    assert got["errors_expected"] > 0, got            # the mismatches really happened


@pytest.mark.parametrize("world", [2, 3, 5])
def test_a_rank_that_leaves_wakes_the_waiters(rendezvous, world):
    got = run(rendezvous, "leave", world)
    assert got["ok_before"] == world                  # a good round first
    assert got["woken"] == world - 1 and got["later_failed"] == world - 1
    assert got["message_differs"] == 0 and got["names_the_rank"], got


def test_ids_are_refused_and_never_reused(rendezvous):
    got = run(rendezvous, "ids")
    assert got["refused"] == 6 and got["accepted"] == 2, got   # world 0, wrong world, rank taken, complete, unknown, other process
    assert got["decoded"] and got["rccl_like_rejected"], got
    assert "already complete" in got["complete_msg"]


@pytest.mark.parametrize("src,hip", [(os.path.join("examples", "connect_four_threads.cpp"), False),
                                     (os.path.join("tests", "cpp", "test_coach_local.cpp"), False),
                                     (os.path.join("tests", "cpp", "test_comm_local.cpp"), True)])
def test_local_comm_programs_compile_and_link(engine_mod, src, hip, tmp_path):
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    exe = os.path.join(tmp_path, "prog")
    cmd = ["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-o", exe,
           "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"]
    if hip:
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        cmd += ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                f"-Wl,-rpath,{os.path.join(rocm, 'lib')}"]
    subprocess.check_call(cmd)
    assert os.path.exists(exe)


def test_bindings_declare_the_local_id(engine_mod):
    assert "az_comm_local_id" in engine_mod.EXPORTS
    assert callable(engine_mod.Engine.comm_local_id)
    assert hasattr(engine_mod._lib, "az_comm_local_id")
    src = open(os.path.join(ROOT, "rust", "az-engine-sys", "src", "lib.rs")).read()
    assert "pub fn comm_local_id(" in src

"""The in-process communicator (az_comm_local_id) on one MI355X: 2..4 engines of one process on device 0, one host thread per rank,
through the collectives of the sharded Coach loop.  The multi-rank cases run in a child process (tests/cpp/test_comm_local.cpp,
tests/cpp/test_coach_local.cpp) with a watchdog of its own and a subprocess timeout, so a regression fails a test instead of
stalling the suite; one case runs through Python threads to exercise the binding."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(engine_mod, src, out, hip=False):
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-o", out,
           "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"]
    if hip:
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        cmd += ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                f"-Wl,-rpath,{os.path.join(rocm, 'lib')}"]
    subprocess.check_call(cmd)
    return out


@pytest.fixture(scope="module")
def exe(engine_mod, tmp_path_factory):
    return _compile(engine_mod, os.path.join("tests", "cpp", "test_comm_local.cpp"), str(tmp_path_factory.mktemp("local") / "test_comm_local"), hip=True)


def run(exe, *args, timeout=200):
    # the binary's own watchdog (150 s) exits non-zero first; this limit only catches a process that cannot even do that
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    got = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert got["bad"] == 0, (got, p.stderr[-3000:])
    return got


@pytest.mark.parametrize("world", [2, 3, 4])
def test_gather_samples(exe, world):
    """Ragged counts (a zero-count rank included), dst_rank 0 / last / -1, host and device buffers on both sides: every receiving rank
    gets the rank-order concatenation bit for bit, every rank the right counts_out, a non-receiver count 0."""
    got = run(exe, "gather", world)
    assert got["cases"] == 12


@pytest.mark.parametrize("world", [2, 3])
def test_refusals_before_posting(exe, world):
    """A receiver too small on one rank, missing local buffers on one rank, ranks that disagree on dst_rank: every rank returns
    AZ_ERR_BAD_ARGUMENT with the same message, and a correct gather on the same communicator follows."""
    got = run(exe, "refuse", world)
    assert got["refusals"] == 3 and got["recovered"] == 3, got


@pytest.mark.parametrize("world", [2, 4])
def test_allreduce_u64(exe, world):
    got = run(exe, "allreduce", world)
    assert got["checked"] == 3 * world


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_arena_tally(exe, world):
    """A 24-game arena (hash nets) split into shards -- even ones, and ones where rank 0's shard is empty -- played from the initial
    board and from a finished one: every rank's out_wld equals the unsharded call's, each shard's results equal the unsharded slice."""
    got = run(exe, "arena", world)
    assert got["cases"] == 4


def test_misuse_fails_on_every_rank_and_never_hangs(exe):
    """Mismatched collectives and different n (one message on every rank, then a correct gather), a rank that calls az_comm_destroy
    while its peers wait (they wake with the error; later calls fail at once), a duplicate rank, a wrong world, a reused id, an unknown
    serial, an engine that already has a communicator, and az_destroy of a member without az_comm_destroy."""
    got = run(exe, "misuse")
    assert got["checks"] == 18, got


def test_coach_in_one_process_matches_the_unsharded_run(engine_mod, tmp_path):
    """test_coach.cpp's miniature (C = 128, 2 iterations, 48 episodes, 25 sims, 16 arena games), unsharded and then at world 2 and 3 in
    ONE process (an engine and a thread per rank, one device, identical options): every file rank 0 writes -- the .examples files,
    the .aznet files and coach.state -- is byte-identical to the unsharded run's, and every rank's per-iteration report equals it."""
    prog = _compile(engine_mod, os.path.join("tests", "cpp", "test_coach_local.cpp"), os.path.join(tmp_path, "test_coach_local"))
    d = os.path.join(tmp_path, "runs")
    p = subprocess.run([prog, d, "11", "2", "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=450)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    got = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    plain = got["plain"]
    assert len(plain) == 2 and all(r["samples"] > 0 and r["nwins"] + r["pwins"] + r["draws"] == 16 for r in plain)
    files = sorted(os.listdir(os.path.join(d, "plain")))
    assert {"0.examples", "1.examples", "1.aznet", "coach.state"} <= set(files), files
    for world in ("2", "3"):
        reps = got["worlds"][world]
        assert len(reps) == int(world)
        for rank, rep in enumerate(reps):
            assert rep == plain, (world, rank)
        wdir = os.path.join(d, "w" + world)
        assert sorted(os.listdir(wdir)) == files
        for f in files:
            with open(os.path.join(d, "plain", f), "rb") as x, open(os.path.join(wdir, f), "rb") as y:
                assert x.read() == y.read(), (world, f)
    print("coach miniature wall time (s):", got["seconds"])


def test_python_threads_drive_one_engine_each(engine_mod):
    """The binding: Engine.comm_local_id, then three Python threads (ctypes releases the GIL), one engine each, through a gather to
    every rank, an all-reduce and a mismatch.  Daemon threads joined with a timeout: a hang fails the test instead of the suite."""
    world = 3
    es = [engine_mod.Engine(device=0, max_batch=64, net_channels=128) for _ in range(world)]
    try:
        for e in es:
            e.set_option("search_graph", 0)
        uid = es[0].comm_local_id(world)
        assert uid.dtype == np.uint8 and uid.size == engine_mod.COMM_ID_BYTES
        rng = np.random.default_rng(3)
        counts = [7, 0, 12]
        loc = [(rng.integers(0, 2**63, (n, 2), dtype=np.uint64), rng.random((n, 7), dtype=np.float32), rng.random(n, dtype=np.float32))
               for n in counts]
        res, errs = [None] * world, [None] * world

        def rank_main(r):
            try:
                es[r].comm_init(r, world, uid)
                gs, gp, gz, cnt = es[r].gather_samples(*loc[r], dst=-1, is_dst=True, capacity=sum(counts))
                tally = es[r].allreduce_u64(np.array([r, 2**64 - 1, 5], np.uint64))
                try:
                    if r == 0:
                        es[r].allreduce_u64(np.array([1, 2], np.uint64))
                    else:
                        es[r].allreduce_u64(np.array([1, 2, 3], np.uint64))
                    mismatch = None
                except engine_mod.AzError as ex:
                    mismatch = str(ex)
                res[r] = (gs, gp, gz, cnt, tally, mismatch)
                es[r].comm_destroy()
            except Exception as ex:  # noqa: BLE001 -- reported below
                errs[r] = ex

        th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in th), "a rank hung"
        assert errs == [None] * world, errs
        want = [np.concatenate([x[i] for x in loc]) for i in range(3)]
        for r in range(world):
            gs, gp, gz, cnt, tally, mismatch = res[r]
            assert cnt.tolist() == counts
            assert np.array_equal(gs, want[0]) and np.array_equal(gp, want[1]) and np.array_equal(gz, want[2])
            assert tally.tolist() == [0 + 1 + 2, 2**64 - 3, 15]          # (2^64 - 1) x 3 wraps
            assert mismatch is not None and "different n" in mismatch and mismatch == res[0][5]
    finally:
        for e in es:
            e.close()

"""The shared tree batch (az_tree_share): many host threads, one slot each, their get_action_prob calls coalesced into batched
searches.  Each caller's result must be what a 1-game az_tree returns for the same calls -- checked against the oracle's
Coach::execute_episode (hash net) and against today's 1-game path bit for bit (conv net), whatever shared the batches."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SALT = 0x51ED27
AZ_OK, AZ_ERR_BAD_ARGUMENT, AZ_ERR_CAPACITY, AZ_ERR_TERMINAL_ROOT = 0, 1, 2, 5


@pytest.fixture(scope="module")
def exe(engine_mod, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shared") / "test_shared_tree")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_shared_tree.cpp"), "-o", out, "-L", libdir, "-laz_engine",
                           f"-Wl,-rpath,{libdir}"])
    return out


def run(exe, *args, timeout=300):
    # the binary's own watchdog (240 s) exits non-zero first; this limit only catches a process that cannot even do that
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def check_against_oracle(got, ref, episodes):
    off = 0
    for ep in range(episodes):
        n = int(ref["game_len"][ep])
        e = got["episodes"][ep]
        assert e["moves"] == ref["moves"][ep, :n].tolist(), ep
        assert e["samples"] == 2 * n, ep
        z = ref["zs"][off:off + 2 * n].astype(np.float64).sum()
        assert abs(e["zsum"] - z) < 1e-6, ep
        assert abs(e["pisum"] - ref["pis"][off:off + 2 * n].astype(np.float64).sum()) < 1e-3, ep
        off += 2 * n


@pytest.mark.parametrize("window_us", [0, 200])
def test_hash_net_64_threads_match_the_oracle(exe, oracle, window_us):
    episodes, sims = 256, 25
    got = run(exe, "hash", 64, 64, episodes, sims, 1, window_us)
    ref = oracle.selfplay(episodes, sims, net_kind=oracle.NET_HASH, salt=1234 + 10 * MODEL_SALT, seed=17, threads=8)
    check_against_oracle(got, ref, episodes)
    batches, requests, largest, by_window = got["share_stats"]
    assert requests == sum(len(e["moves"]) for e in got["episodes"])
    assert largest <= 64
    if window_us == 0:
        assert by_window == 0
        assert requests / batches >= 32, got["share_stats"]       # the calls really were coalesced


def test_hash_net_two_sim_threads_match_the_oracle(exe, oracle):
    episodes, sims = 64, 26
    got = run(exe, "hash", 64, 64, episodes, sims, 2, 0)
    ref = oracle.selfplay(episodes, sims, net_kind=oracle.NET_HASH, salt=1234 + 10 * MODEL_SALT, seed=17, threads=8, sim_threads=2)
    check_against_oracle(got, ref, episodes)


def test_conv_net_64_threads_bit_identical_to_one_game_trees(exe):
    got = run(exe, "conv", 64, 64, 25)
    assert got["moves"] > 64
    assert got["moves_mismatch"] == 0 and got["pi_mismatch"] == 0, got
    batches, requests, _, _ = got["share_stats"]
    assert requests / batches > 8, got["share_stats"]


def test_terminal_root_fails_only_its_request(exe):
    got = run(exe, "errors")
    assert got["batches"] == 1                        # every request of the run shared one batch
    assert got["terminal_status"] == AZ_ERR_TERMINAL_ROOT and got["terminal_msg_len"] > 0
    assert got["others_ok"] == got["others"] == 7
    assert got["others_identical"] == 7


def test_contract(exe):
    got = run(exe, "contract")
    assert got["plain_acquire"] == AZ_ERR_BAD_ARGUMENT
    assert got["get_action_prob"] == AZ_ERR_BAD_ARGUMENT and got["reset"] == AZ_ERR_BAD_ARGUMENT
    assert got["acquire_all"] == AZ_OK and sorted(got["slots"]) == [0, 1, 2, 3]
    assert got["acquire_over"] == AZ_ERR_CAPACITY
    assert got["out_of_range"] == AZ_ERR_BAD_ARGUMENT and got["negative"] == AZ_ERR_BAD_ARGUMENT
    assert got["not_held"] == AZ_ERR_BAD_ARGUMENT
    assert got["double_release"] == AZ_ERR_BAD_ARGUMENT and got["release_range"] == AZ_ERR_BAD_ARGUMENT
    assert got["own"] == AZ_OK and abs(got["own_pi_sum"] - 1.0) < 1e-5


def test_python_threads_match_the_oracle(engine, engine_mod, oracle):
    """16 threading.Threads, one slot each, drive TreeBatch.slot_get_action_prob with the hash net; every move's pi / counts / Q
    equal the oracle's AsyncMcts::get_action_prob on the same position."""
    n, sims, seed = 16, 25, 3
    tb = engine_mod.TreeBatch(engine, n, reserve=oracle.default_reserve(sims), num_sims=sims, max_depth=1000, model_id=10, cpuct=1)
    try:
        tb.share(0)
        oracle_lock = threading.Lock()
        results, errors = [None] * n, [None] * n

        def worker(w):
            slot = None
            try:
                slot = tb.slot_acquire()
                with oracle_lock:
                    ot = oracle.Tree(sims, net_kind=oracle.NET_HASH, salt=1234 + 10 * MODEL_SALT)
                rng = np.random.default_rng(w)
                state, bad, moves = (0, 0), [], 0
                for ply in range(42):
                    temp = 1.0 if ply < 15 else 0.0
                    pi, counts, q = tb.slot_get_action_prob(slot, state, temp, seed=seed, game_id=500 + w)
                    with oracle_lock:
                        opi, ocnt, oq = ot.get_action_prob(state[0], state[1], temp, seed=seed, game_id=500 + w)
                    if not (np.array_equal(pi, opi) and np.array_equal(counts, ocnt) and np.array_equal(q, oq)):
                        bad.append(ply)
                    moves += 1
                    a = int(rng.choice([c for c in range(7) if opi[c] > 0]))
                    nxt = oracle.c4_play(state[0], state[1], a)
                    if oracle.c4_ended(*nxt) != 0.0:
                        break
                    state = nxt
                with oracle_lock:
                    ot.close()
                results[w] = (moves, bad)
            except Exception as ex:          # noqa: BLE001 -- reported by the main thread
                errors[w] = repr(ex)
            finally:
                if slot is not None:
                    tb.slot_release(slot)        # a failed worker must not keep the others' batches waiting

        threads = [threading.Thread(target=worker, args=(w,), daemon=True) for w in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=240)
        assert not any(t.is_alive() for t in threads), "a slot call never returned"
        assert errors == [None] * n, errors
        assert all(r[1] == [] for r in results), results
        st = tb.share_stats()
        assert st["requests"] == sum(r[0] for r in results)
        assert st["batches"] < st["requests"]
        with pytest.raises(engine_mod.AzError) as ex:
            tb.get_action_prob(np.zeros((n, 2), np.uint64), 1.0)
        assert ex.value.status == AZ_ERR_BAD_ARGUMENT
    finally:
        tb.close()

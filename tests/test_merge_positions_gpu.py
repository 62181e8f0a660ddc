"""Position averaging on the GPU (az_samples_merge, include/az_engine.h): every output -- count, states, boards, pis,
zs, counts -- bit for bit against the numpy twin (tests/merge_twin.py), at the sizes where each mechanism of the kernels can go wrong; the
input routes, the refusals, purity, and both Coaches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch                   # before the engine library is loaded: torch brings its own HIP runtime, and a process wants one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feature_gpu as fg       # noqa: E402
import merge_twin as mg        # noqa: E402
import mirror_twin as mt       # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("states", "boards", "pis", "zs", "counts")
SENTINEL = {"states": 0xA5A5A5A5A5A5A5A5, "boards": 123.0, "pis": 123.0, "zs": 123.0, "counts": 0xDEADBEEF}
SHAPE = {"states": ((2,), np.uint64), "boards": ((2, 6, 7), np.float32), "pis": ((7,), np.float32), "zs": ((), np.float32),
         "counts": ((), np.uint32)}


def same(got, want, keys=KEYS):
    """the engine's dict against the twin's: count and every array, as bytes"""
    assert got["count"] == want["count"], (got["count"], want["count"])
    for k in keys:
        assert fg.same_rows(np.asarray(got[k]), np.asarray(want[k])), k


def sentinel_outputs(n, keys=KEYS):
    return {k: np.full((n,) + SHAPE[k][0], SENTINEL[k], SHAPE[k][1]) for k in keys}


def raw_merge(e, em, pis, zs, *, states=None, boards=None, flags=0, capacity=None, out=None, n=None):
    """az_samples_merge through the bare ABI: (status, dst.count, out).  `out` holds the dst arrays (numpy or torch; a missing key is NULL)."""
    n = len(zs) if n is None else n
    capacity = n if capacity is None else capacity
    out = sentinel_outputs(max(capacity, 1)) if out is None else out
    src = em.az_samples(n, n, em._as_ptr(states), em._as_ptr(boards), em._as_ptr(pis), em._as_ptr(zs), None, None)
    dst = em.az_samples(capacity, -7, em._as_ptr(out.get("states")), em._as_ptr(out.get("boards")), em._as_ptr(out.get("pis")),
                        em._as_ptr(out.get("zs")), None, None)
    st = e._lib.az_samples_merge(e._h, em.C.byref(src), flags, em.C.byref(dst), em._as_ptr(out.get("counts")))
    return st, int(dst.count), out


@pytest.fixture(scope="module")
def pool():
    """3000 distinct legal positions, and 70 000 tuples drawn from them with replacement, with the twin's answers (computed once)."""
    rng = np.random.default_rng(2024)
    pos = mg.random_positions(rng, 3000)
    idx = rng.integers(0, 3000, 70000)
    pis, zs = mg.random_targets(rng, 70000)
    heavy = {"states": np.ascontiguousarray(pos[idx]), "pis": pis, "zs": zs}
    return {"pos": pos, "heavy": heavy, "plain": mg.merge(pis, zs, states=heavy["states"]),
            "canonical": mg.merge(pis, zs, states=heavy["states"], canonical=True)}


@pytest.fixture(scope="module")
def engine3(engine_mod):
    """The seam's second game (AZ_GAME_CONNECT_THREE)."""
    yield from fg.connect_three_engine(engine_mod)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_distinct_positions_come_back_verbatim(engine, pool, n):
    """wave and workgroup boundaries; a set without duplicates is unchanged"""
    rng = np.random.default_rng(n)
    states = pool["pos"][rng.permutation(3000)[:n]]
    pis, zs = mg.random_targets(rng, n)
    if n:
        pis[0, 0] = np.array([3], np.uint32).view(np.float32)[0]          # a denormal goes through untouched
    got = engine.merge_samples(pis, zs, states=states, want_boards=True)
    same(got, mg.merge(pis, zs, states=states))
    assert got["count"] == n and fg.same_rows(got["states"], states) and fg.same_rows(got["pis"], pis) and fg.same_rows(got["zs"], zs)
    assert (got["counts"] == 1).all()


def test_one_group_of_a_thousand(engine, pool):
    """maximum same-address contention"""
    rng = np.random.default_rng(1)
    pis, zs = mg.random_targets(rng, 1000)
    for state in (np.zeros(2, np.uint64), pool["pos"][17]):
        states = np.tile(state, (1000, 1))
        got = engine.merge_samples(pis, zs, states=states, want_boards=True)
        same(got, mg.merge(pis, zs, states=states))
        assert got["count"] == 1 and got["counts"].tolist() == [1000]


def test_heavy_duplication(engine, pool):
    """several workgroups, probe chains, a scan across blocks, first occurrences in shuffled order"""
    h = pool["heavy"]
    for canonical in (False, True):
        want = pool["canonical" if canonical else "plain"]
        got = engine.merge_samples(h["pis"], h["zs"], states=h["states"], canonical=canonical, want_boards=True)
        same(got, want)
        assert got["count"] <= 3000 and int(got["counts"].sum()) == 70000 and got["counts"].max() > 1
    assert pool["canonical"]["count"] <= pool["plain"]["count"]
    first = {}
    for i, s in enumerate(map(tuple, h["states"].tolist())):
        first.setdefault(s, i)
    assert [tuple(s) for s in pool["plain"]["states"].tolist()] == sorted(first, key=first.get)      # the order really is first occurrence


def test_a_window_of_700_000(engine, pool):
    """The paths only a large input takes.  2735 rounds of 256 tuples on 2048 accumulate workgroups: 687 of them run two rounds with one LDS
    table.  Every tuple is one of four hot positions with probability 1/2, else one of 3000: a round leaves about 129 slots of the table used,
    either side of the 128 at which the next round first empties it, so both the carried and the flushed table run.  The per-block totals
    (2735) take three chunks of the 1024-wide block scan, with a carry."""
    rng = np.random.default_rng(77)
    n = 700000
    hot = rng.random(n) < 0.5
    idx = np.where(hot, rng.integers(0, 4, n), rng.integers(0, 3000, n))
    states = np.ascontiguousarray(pool["pos"][idx])
    pis, zs = mg.random_targets(rng, n)
    used = [len(set(idx[r * 256:(r + 1) * 256].tolist())) for r in range(2048)]          # slots a workgroup's first round leaves used
    assert min(used) <= 128 < max(used)
    for canonical in (False, True):
        want = mg.merge(pis, zs, states=states, canonical=canonical)
        got = engine.merge_samples(pis, zs, states=states, canonical=canonical, want_boards=True)
        same(got, want)
        assert got["count"] <= 3000 and int(got["counts"].sum()) == n and got["counts"].max() > n // 10


def test_a_permutation_keeps_the_groups(engine, pool):
    h, want = pool["heavy"], pool["plain"]
    perm = np.random.default_rng(3).permutation(70000)
    pis, zs, states = h["pis"][perm], h["zs"][perm], np.ascontiguousarray(h["states"][perm])
    got = engine.merge_samples(pis, zs, states=states, want_boards=True)
    same(got, mg.merge(pis, zs, states=states))                 # the twin's order for the permuted input
    assert not fg.same_rows(got["states"], want["states"])
    # the same multiset of (state, mean pi, mean z, count): the sums do not depend on the order of the addends
    rows = lambda r: sorted(zip(map(tuple, r["states"].tolist()), r["pis"].view(np.uint32).tolist(), r["zs"].view(np.uint32).tolist(), r["counts"].tolist()))
    assert rows(got) == rows(want)


@pytest.mark.parametrize("symmetries", [False, True])
def test_selfplay_tuples(engine, symmetries):
    sp = fg.run_selfplay(engine, 25, seed=6, symmetries=symmetries)
    n = sp["count"]
    states, pis, zs = np.array(sp["states"]), np.array(sp["pis"]), np.array(sp["zs"])
    for canonical in (False, True):
        got = engine.merge_samples(pis, zs, states=states, canonical=canonical, want_boards=True)
        same(got, mg.merge(pis, zs, states=states, canonical=canonical))
        m = got["count"]
        print("self-play: n %d, m %d (%.3f), canonical %d, symmetries %d" % (n, m, m / n, canonical, symmetries))
        assert 0 < m < n and int(got["counts"].sum()) == n          # the empty board alone guarantees m < n
        if canonical and symmetries:
            odd = got["counts"] % 2 == 1
            assert fg.same_rows(mt.mirror_batch(got["states"][odd]), got["states"][odd])       # only self-symmetric positions may be odd
    # from the features the self-play call wrote: the same groups
    viab = engine.merge_samples(pis, zs, boards=np.array(sp["boards"]), want_boards=True)
    same(viab, mg.merge(pis, zs, states=states))


def test_input_routes(engine, engine_mod, pool):
    h, n = pool["heavy"], 5000
    states, pis, zs = h["states"][:n], h["pis"][:n], h["zs"][:n]
    want = mg.merge(pis, zs, states=states, canonical=True)
    boards = mt.states_to_boards(states)
    same(engine.merge_samples(pis, zs, boards=boards, canonical=True, want_boards=True), want)
    # device pointers in
    dev = torch.device("cuda", 0)
    t = {"states": torch.from_numpy(states.view(np.int64).copy()).to(dev), "pis": torch.from_numpy(pis.copy()).to(dev),
         "zs": torch.from_numpy(zs.copy()).to(dev), "boards": torch.from_numpy(boards).to(dev)}
    same(engine.merge_samples(t["pis"], t["zs"], states=t["states"], canonical=True, want_boards=True), want)
    same(engine.merge_samples(t["pis"], t["zs"], boards=t["boards"], canonical=True, want_boards=True), want)
    # device pointers out
    out = {"states": torch.zeros((n, 2), dtype=torch.int64, device=dev), "boards": torch.zeros((n, 2, 6, 7), device=dev),
           "pis": torch.zeros((n, 7), device=dev), "zs": torch.zeros(n, device=dev), "counts": torch.zeros(n, dtype=torch.int32, device=dev)}
    st, m, _ = raw_merge(engine, engine_mod, t["pis"], t["zs"], states=t["states"], flags=1, out=out, n=n)
    assert st == 0
    got = {"count": m, "states": out["states"].cpu().numpy().view(np.uint64)[:m], "boards": out["boards"].cpu().numpy()[:m],
           "pis": out["pis"].cpu().numpy()[:m], "zs": out["zs"].cpu().numpy()[:m], "counts": out["counts"].cpu().numpy().view(np.uint32)[:m]}
    same(got, want)
    # dst->states NULL with dst->boards set, the reverse, and no counts
    for keys in (("boards", "pis", "zs", "counts"), ("states", "pis", "zs", "counts"), ("pis", "zs")):
        out = sentinel_outputs(n, keys)
        st, m, _ = raw_merge(engine, engine_mod, pis, zs, boards=boards, flags=1, out=out)
        assert st == 0 and m == want["count"]
        same(dict(count=m, **{k: v[:m] for k, v in out.items()}), want, keys)
        for k in keys:                                            # nothing behind the m-th row is touched
            assert (out[k][m:] == np.asarray(SENTINEL[k]).astype(SHAPE[k][1])).all(), k


def test_connect_three(engine3, pool):
    h = pool["heavy"]
    n = 5000
    states, pis, zs = h["states"][:n], h["pis"][:n], h["zs"][:n]
    for canonical in (False, True):
        same(engine3.merge_samples(pis, zs, states=states, canonical=canonical, want_boards=True), mg.merge(pis, zs, states=states, canonical=canonical))
    sp = fg.run_selfplay(engine3, 25, seed=6, n_games=40, symmetries=True)
    same(engine3.merge_samples(sp["pis"], sp["zs"], boards=sp["boards"], canonical=True, want_boards=True),
         mg.merge(sp["pis"], sp["zs"], states=sp["states"], canonical=True))


def test_refusals(engine, engine_mod, pool):
    n = 300
    states, pis, zs = pool["pos"][:n].copy(), *mg.random_targets(np.random.default_rng(9), n)
    boards = mt.states_to_boards(states)

    def changed(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a

    def refused(pis=pis, zs=zs, **kw):
        twin_kw = {k: kw[k] for k in ("states", "boards", "capacity", "flags") if k in kw}
        if "out" not in kw:
            assert mg.refusal(pis, zs, **twin_kw) is not None
        st, cnt, out = raw_merge(engine, engine_mod, pis, zs, **kw)
        assert st == fg.AZ_ERR_BAD_ARGUMENT and cnt == -7, (st, cnt)
        for k, v in out.items():
            if not (v is pis):
                assert (v == np.asarray(SENTINEL[k]).astype(SHAPE[k][1])).all(), k
    refused(pis=changed(pis, (299, 6), 1.5), states=states)
    refused(zs=changed(zs, 100, -2.0), states=states)
    refused(pis=changed(pis, (64, 0), np.nan), states=states)
    refused(zs=changed(zs, 0, np.nan), states=states)
    refused(states=changed(states, 5, (1, 1)))                                                    # overlapping stones
    refused(states=changed(states, (7, 1), states[7, 1] | np.uint64(1 << (3 * 7 + 6))))            # a stone at bit col * 7 + 6
    refused(boards=changed(boards, (3, 0, 0, 0), 0.5))
    refused(boards=changed(changed(boards, (3, 0, 0, 0), 1.0), (3, 1, 0, 0), 1.0))
    refused(states=states, capacity=n - 1)
    refused(states=states, flags=2)
    out = sentinel_outputs(n)
    out["pis"] = pis                                                                              # dst->pis == src->pis
    before = pis.copy()
    refused(states=states, out=out)
    assert fg.same_rows(pis, before)
    # an open self-play session; after selfplay_end the same call succeeds
    engine.selfplay_begin(4, 10, 10, seed=1)
    try:
        refused(states=states, out=sentinel_outputs(n))
    finally:
        engine.selfplay_end()
    st, m, out = raw_merge(engine, engine_mod, pis, zs, states=states)
    assert st == 0 and m == n and fg.same_rows(out["pis"][:n], pis)


def test_purity(engine, pool):
    h = pool["heavy"]
    before = fg.other_entry_points(engine)
    engine.reset_stats()
    zero = engine.stats()
    same(engine.merge_samples(h["pis"], h["zs"], states=h["states"], want_boards=True), pool["plain"])
    st = engine.stats()
    assert {k: v for k, v in st.items() if k != "device_ms"} == {k: v for k, v in zero.items() if k != "device_ms"}
    fg.assert_same_outputs(fg.other_entry_points(engine), before)


@pytest.mark.parametrize("canonical", [False, True])
def test_python_and_cpp_coach_agree(engine_mod, tmp_path, canonical):
    """fg.run_coach_pair in miniature with merge_positions on both hosts: same report, byte-identical files; history stays raw (0.examples is
    the control run's), training saw another set (1.aznet is not)."""
    from alphazero_rs_amd.coach import Coach
    C, seed = 128, 11
    dirs = {k: os.path.join(tmp_path, k) for k in ("py", "cpp", "plain")}

    def run_py(d, merge):
        e = engine_mod.Engine(device=0, max_batch=256, net_channels=C)
        try:
            e.net_init_random(0, 3)
            e.set_option("train_epochs", 1)
            coach = Coach.setup(e, d, 1000000, 0.55, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1, log=lambda m: None)
            coach.merge_positions, coach.merge_canonical = merge, merge and canonical
            return coach.learn(seed=seed)
        finally:
            e.close()
    rep, plain = run_py(dirs["py"], True), run_py(dirs["plain"], False)
    exe = os.path.join(tmp_path, "test_coach_merge")
    libdir = os.path.dirname(engine_mod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coach_merge.cpp"),
                           "-o", exe, "-L", libdir, "-laz_engine", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, dirs["cpp"], str(C), str(seed), "1", "1" if canonical else "0"], check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    crep = json.loads([l for l in out.strip().splitlines() if l.startswith("[")][-1])
    assert len(rep) == len(crep) == len(plain) == 1
    for k in fg.REPORT_KEYS + ("samples_raw",):
        assert rep[0][k] == crep[0][k], k
    print("coach: samples %d of %d raw (canonical %d)" % (rep[0]["samples"], rep[0]["samples_raw"], canonical))
    assert rep[0]["samples"] < rep[0]["samples_raw"] == plain[0]["samples"] == plain[0]["samples_raw"]
    fg.compare_directories(dirs["py"], dirs["cpp"])
    read = lambda d, f: open(os.path.join(dirs[d], f), "rb").read()
    assert read("py", "0.examples") == read("plain", "0.examples")
    assert read("py", "1.aznet") != read("plain", "1.aznet")

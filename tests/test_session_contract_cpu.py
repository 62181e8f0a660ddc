"""tests/session_contract.py is CLOSED-WORLD: every export of include/az_engine.h and every az_set_option key of the shipped library has
exactly one row, so an entry or a key added later has to be classified -- refused or inert beside an open self-play session -- before
the suite passes.  No GPU here: the header and az_set_option's source are parsed."""
import collections
import os
import re

import session_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    """The exports of include/az_engine.h, parsed as tests/test_abi_cpu.py parses them."""
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(az_[a-z_0-9]+)\s*\(", hdr)))


def shipped_option_keys():
    """The keys az_set_option of libaz_engine.so names: its is("...") tests and the first column of its key tables, without the branch
    that only the diagnostic library compiles (#ifdef AZ_DIAG ... #else)."""
    src = open(os.path.join(ROOT, "alphazero-rs_amd", "csrc", "az_engine.hip")).read()
    body = src[src.index("az_status az_set_option("):]
    body = body[:body.index("\naz_status az_get_stats(")]
    body = re.sub(r"#ifdef AZ_DIAG.*?#else", "", body, flags=re.S)
    keys = set(re.findall(r'\bis\("([a-z0-9_]+)"\)', body)) | set(re.findall(r'\{"([a-z0-9_]+)",', body))
    assert len(keys) > 60 and "eval_dedup" in keys and "train_ema_decay_e9" in keys and "gumbel_m" in keys
    return sorted(keys)


def test_every_export_has_exactly_one_row():
    names = [r.name for r in sc.EXPORTS]
    twice = [n for n, k in collections.Counter(names).items() if k > 1]
    assert not twice, "listed twice: %s" % twice
    decl = declared_symbols()
    assert sorted(names) == decl, ("not classified: %s; not an export: %s" % (sorted(set(decl) - set(names)), sorted(set(names) - set(decl))))


def test_every_option_key_has_exactly_one_row():
    names = [r.name for r in sc.OPTIONS]
    twice = [n for n, k in collections.Counter(names).items() if k > 1]
    assert not twice, "listed twice: %s" % twice
    keys = shipped_option_keys()
    assert sorted(names) == keys, ("not classified: %s; not a key: %s" % (sorted(set(keys) - set(names)), sorted(set(names) - set(keys))))


def test_rows_are_well_formed():
    for r in sc.ROWS:
        assert r.cls in sc.CLASSES, r
        assert (r.call is None) == (r.cls == sc.OWN), r                 # everything but the session's own entries can be called
    assert sorted(r.name for r in sc.ROWS if r.cls == sc.OWN) == sorted(sc.OWN_ENTRIES)
    assert all(r.cls in (sc.REFUSED, sc.INERT) for r in sc.OPTIONS)     # a key has no model id
    # the minimum the contract names: nothing that searches, rewrites the session's model or reshapes the cache is inert
    by_name = {r.name: r.cls for r in sc.ROWS}
    for n in ("az_arena", "az_tournament", "az_tree_get_action_prob", "az_tree_slot_get_action_prob", "az_tree_share", "az_selfplay",
              "conv2_table", "eval_dedup", "eval_cache_log2", "eval_cache_persist", "eval_cache_max_stones", "selfplay_async",
              "selfplay_async_launches", "selfplay_async_iters", "net_fp8", "eval_mirror"):
        assert by_name[n] == sc.REFUSED, n
    for n in ("az_net_free", "az_net_set_params", "az_net_init_random", "az_net_load", "az_net_set_kind", "az_net_train", "az_net_train_end"):
        assert by_name[n] == sc.BY_MODEL, n


def test_the_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    at = hdr.index("THE SESSION CONTRACT")
    assert at < hdr.index("az_status az_selfplay_begin(")                # next to the entry it is about
    para = hdr[at:hdr.index("az_status az_selfplay_begin(")]
    for word in ("REFUSED", "BY MODEL", "INERT", "AZ_ERR_BAD_ARGUMENT", "az_last_error", "tests/session_contract.py", "RESTART"):
        assert word in para, word
    # every entry and key the paragraph names as refused or by-model is of that class in the table
    by_name = {r.name: r.cls for r in sc.ROWS}
    refused = para[para.index("REFUSED"):para.index("BY MODEL")]
    for key in re.findall(r'"([a-z0-9_]+)"', refused):
        assert by_name[key] == sc.REFUSED, key
    by_model = para[para.index("BY MODEL"):para.index("INERT")]
    for name in re.findall(r"\baz_net_[a-z_]+", by_model):
        assert by_name[name] == sc.BY_MODEL, name
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "session contract" in text.lower() and "tests/session_contract.py" in text, doc

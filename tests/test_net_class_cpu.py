"""az_net_class and the two class entry points: include/az_engine.h, alphazero-rs_amd/engine.py, include/az_host.hpp and the Coach
hosts agree (no GPU: the header is parsed, the library only loaded)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_class_values_match_the_header(engine_mod):
    m = re.search(r"typedef enum\s*\{([^}]*)\}\s*az_net_class\s*;", _header())
    assert m, "az_net_class is not declared"
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in m.group(1).split(",") if item.strip())}
    assert vals == {"AZ_NET_CLASS_ENGINE": -1, "AZ_NET_CLASS_BF16": 0, "AZ_NET_CLASS_FP8": 1}
    assert (engine_mod.NET_CLASS_ENGINE, engine_mod.NET_CLASS_BF16, engine_mod.NET_CLASS_FP8) == (-1, 0, 1)


def test_class_prototypes_match_the_binding(engine_mod):
    """The header's prototypes against the ctypes signatures load_library installs, argument by argument."""
    hdr = _header()
    ctype = {"az_engine*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int32_t*": ctypes.POINTER(ctypes.c_int32)}
    lib = ctypes.CDLL(engine_mod.LIB_PATH)
    bound = engine_mod._lib
    for name, nargs in (("az_net_set_class", 3), ("az_net_get_class", 4)):
        m = re.search(r"\baz_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [re.match(r"(.*?)\s*\b[A-Za-z_0-9]+$", a.strip()).group(1).replace(" ", "") for a in m.group(1).split(",")]
        assert len(args) == nargs
        fn = getattr(bound, name)
        assert fn.restype is ctypes.c_int32 and list(fn.argtypes) == [ctype[a] for a in args], (name, args, fn.argtypes)
        assert hasattr(lib, name) and name in engine_mod.EXPORTS
    assert {"net_set_class", "net_class"} <= set(dir(engine_mod.Engine))
    assert list(inspect.signature(engine_mod.Engine.net_set_class).parameters) == ["self", "model_id", "net_class"]


def test_hosts_carry_the_knob():
    """Both Coach hosts and both examples know selfplay_class; the C++ host mirrors the two entry points."""
    host = open(os.path.join(ROOT, "include", "az_host.hpp")).read()
    for needle in ("az_net_set_class(", "az_net_get_class(", "az_net_class selfplay_class = AZ_NET_CLASS_ENGINE"):
        assert needle in host, needle
    coach = open(os.path.join(ROOT, "alphazero-rs_amd", "coach.py")).read()
    assert "self.selfplay_class = -1" in coach and "net_set_class" in coach
    assert "--selfplay-fp8" in open(os.path.join(ROOT, "examples", "connect_four.py")).read()
    assert "selfplay_class" in open(os.path.join(ROOT, "examples", "connect_four.cpp")).read()


def test_python_coach_default_makes_no_class_call(tmp_path):
    """Coach.setup leaves selfplay_class at ENGINE; learn() with it never touches net_set_class (an engine without the method works)."""
    from alphazero_rs_amd.coach import Coach

    class NoEngine:
        pass
    c = Coach.setup(NoEngine(), str(tmp_path), 1000, 0.55, 15, 3, 1000, 1, 4, 4, 1, 4, 25, 1, 100, 1, log=lambda m: None)
    assert c.selfplay_class == -1

"""The environment switches of the C++ library (csrc/lg_switches.h): read only through the header's checked readers, each one listed in its table and in
INTEGRATION.md, and a value outside the accepted set refused by the call that reads it, with the variable and the value named in the error."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
HEADER = os.path.join(CSRC, "lg_switches.h")
LIB = os.path.join(CSRC, "liblgstep.so")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp"))}


def test_switches_are_read_through_the_header_and_documented():
    src = _sources()
    assert [f for f, s in src.items() if "getenv(" in s and f != "lg_switches.h"] == []
    table = set(re.findall(r'^\s*\{"(LG_\w+)",', src["lg_switches.h"], re.M))
    read = {n for s in src.values() for n in re.findall(r'lg_switch_\w+\(\s*"(LG_\w+)"', s)}
    assert read and read == table, (sorted(read - table), sorted(table - read))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(table) if f"`{n}`" not in doc] == []


def _create_error(monkeypatch, env):
    """lg_create of a small quadruped context under `env`: None when it succeeded (the context is destroyed again), else lg_last_error.  The switches
    are read in front of the device check, so where there is no GPU a value they accept ends in the "no HIP device" error instead."""
    from extended_legged_gym_amd.native import load_library
    from extended_legged_gym_amd.envs.anymal_c.flat.anymal_c_flat_config import AnymalCFlatCfg
    from extended_legged_gym_amd.envs.base.native_config import NativeSetup, load_robot_model
    from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args, parse_sim_params
    cfg = AnymalCFlatCfg()
    cfg.env.num_envs = 16
    sp = parse_sim_params(get_args([]), {"sim": class_to_dict(cfg.sim)})
    setup = NativeSetup(cfg, sp, load_robot_model(cfg.asset), seed=1)
    lib = load_library()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = lib.lg_create(C.byref(setup.cfg), C.byref(setup.model), C.byref(setup.terrain), 0, None)
    if ctx:
        lib.lg_destroy(ctx)
        return None
    return lib.lg_last_error(None).decode()


@pytest.mark.skipif(not os.path.exists(LIB), reason="liblgstep.so not built")
@pytest.mark.parametrize("name,value", [("LG_MESH_DEAL", "01234566"), ("LG_DEAL", "0123456x"), ("LG_MESH_REACH", "2"), ("LG_FUSE", "yes"),
                                        ("LG_LATTICE_CAP", "0")])
def test_lg_create_refuses_a_bad_switch_value(monkeypatch, name, value):
    err = _create_error(monkeypatch, {name: value})
    assert err is not None and name in err and value in err, err


@pytest.mark.skipif(not os.path.exists(LIB), reason="liblgstep.so not built")
@pytest.mark.parametrize("env", [{"LG_DEAL": "0", "LG_MESH_DEAL": "0"}, {"LG_DEAL": "76543210", "LG_MESH_DEAL": "10325476", "LG_MESH_REACH": "0.15"},
                                 {"LG_FUSE": "0", "LG_SPLIT": "1", "LG_LATTICE_CAP": "48"}])
def test_lg_create_accepts_good_switch_values(monkeypatch, env):
    err = _create_error(monkeypatch, env)
    assert err is None or not any(k in err for k in env), err

"""CPU side of the sensors inside the one-call collectors (include/lgsensors.h), the pattern of tests/test_runner_privileged_abi.py: the header's
names, the library's exports and the ctypes mirror agree; the symbol list is disjoint from every other; the four structs' layouts match a C
compiler's; one refused call per entry point that can fail leaves a message that starts with that entry point's name; the Python surface is
there and the runner's `sensor_collection` resolves to "host" without the key; the unit's one kernel (cross-compiled for gfx950) shows no spills,
no scratch and no LDS.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from extended_legged_gym_amd import abi
from tests.test_policy_recurrent_abi import HIPCC, LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
LIB = os.path.join(CSRC, "liblgstep.so")
HEADER = os.path.join(ROOT, "include", "lgsensors.h")


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)          # (the comments speak of other headers' calls)
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", text)))
    assert names == sorted(abi.SENSOR_SYMBOLS), (names, abi.SENSOR_SYMBOLS)
    for other in (abi.RUNNER_SYMBOLS, abi.RUNNER_PRIVILEGED_SYMBOLS, abi.RUNNER_DISTILL_SYMBOLS, abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS,
                  abi.DISTILL_TRAIN_SYMBOLS, abi.DISTILL_RTRAIN_SYMBOLS, abi.ESTIMATOR_TRAIN_SYMBOLS, abi.SYMMETRY_TRAIN_SYMBOLS, abi.PRODUCT_SYMBOLS,
                  abi.ESTIMATOR_SYMBOLS, abi.ESTIMATOR_BF16_SYMBOLS):
        assert not set(names) & set(other)
    plain = abi.declare_runner_distill(abi.declare_runner_privileged(abi.declare_runner(abi.declare_train(abi.declare_policy(abi.declare_product(C.CDLL(LIB)))))))
    for sym in names:
        assert hasattr(plain, sym), sym          # exported
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_sensors(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgsensors.h"', "int main(void) {"]
    for name, cls in abi.SENSOR_STRUCTS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert sorted(abi.SENSOR_STRUCTS) == ["lg_estimation_nets", "lg_estimation_out", "lg_sensor_camera", "lg_sensor_raycaster"]
    for name, cls in abi.SENSOR_STRUCTS.items():
        assert int(got[name]) == C.sizeof(cls), name
        for field, _ in cls._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, (name, field)
    declared = re.findall(r"typedef struct (lg_\w+) \{", open(HEADER).read())
    assert sorted(declared) == sorted(abi.SENSOR_STRUCTS)


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_sensors(abi.declare_runner(abi.declare_policy(C.CDLL(LIB))))
    p = 0x1000          # never read: the NULL handle is refused first
    rows = abi.lg_rollout(*[p] * 11)
    est = abi.lg_estimation_out(*[p] * 5)
    calls = {
        "lg_sensor_rig_create": lambda: lib.lg_sensor_rig_create(None, None, None, None),
        "lg_sensor_rig_set_counter": lambda: lib.lg_sensor_rig_set_counter(None, 0),
        "lg_sensor_step_transition": lambda: lib.lg_sensor_step_transition(None, p, None, None, 0.99, p, p, None),
        "lg_runner_collect_sensors": lambda: lib.lg_runner_collect_sensors(None, None, p, None, p, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None, None,
                                                                          None, None),
        "lg_estimation_rows": lambda: lib.lg_estimation_rows(None, 2, 16, None, None, None, None, 4, 8, p, None, None, None),
        "lg_collect_estimation": lambda: lib.lg_collect_estimation(None, p, None, 4, C.byref(est), None, None),
    }
    quiet = {"lg_sensor_rig_destroy", "lg_sensor_rig_counter", "lg_post_physics_transition", "lg_extra_obs_info"}          # no message of their own: see below
    assert set(calls) | quiet == set(abi.SENSOR_SYMBOLS)
    for name, call in calls.items():
        rc = call()
        assert rc in (abi.LG_ERR_INVALID, None), (name, rc)          # (a create function returns NULL)
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    # the four others: destroy takes NULL, the getter says -1, the two context entries answer a NULL context with LG_ERR_INVALID as lg_step_physics does
    lib.lg_sensor_rig_destroy(None)
    assert lib.lg_sensor_rig_counter(None) == -1
    assert lib.lg_post_physics_transition(None, None, None, 0.99, p, p, None) == abi.LG_ERR_INVALID
    assert lib.lg_extra_obs_info(None, None, None) == abi.LG_ERR_INVALID


def test_python_surface_and_the_runners_default():
    from extended_legged_gym_amd import rl
    from extended_legged_gym_amd.rl import collector, runner, sensors
    assert hasattr(rl, "SensorRig") and all(hasattr(rl.SensorRig, m) for m in ("from_env", "finish", "begin", "step_transition"))
    assert "sensors" in inspect.signature(collector.collect_rollout_tracked).parameters
    sig = inspect.signature(collector.collect_estimation).parameters
    assert sig["one_call"].default is False and sig["actions"].default is None
    assert runner.sensor_collection_mode({}) == "host" and runner.sensor_collection_mode({"sensor_collection": "native"}) == "native"
    with pytest.raises(ValueError, match="sensor_collection"):
        runner.sensor_collection_mode({"sensor_collection": "device"})
    src = inspect.getsource(runner.NativeOnPolicyRunner.__init__)
    assert "sensor_collection_mode(self.cfg)" in src          # the constructor resolves the key through that function
    assert callable(sensors.refusal)
    from extended_legged_gym_amd.utils.helpers import get_args
    assert get_args([]).sensor_collection is None and get_args(["--sensor_collection", "native"]).sensor_collection == "native"
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_estimator
    assert inspect.signature(train_estimator.train).parameters["collect"].default == "host"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_gather_kernel_does_not_spill_and_uses_no_lds(tmp_path):
    """The route of tests/test_runner_privileged_abi.py on csrc/lg_sensors.hip: one kernel, the row gather, and nothing else."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_sensors.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_sensors.hip")], check=True, capture_output=True)
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks, cur = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith("- .agpr_count:") or line.startswith("- .args:"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == "name":
                blocks[m.group(2)] = cur
            elif m.group(2).isdigit():
                cur[m.group(1)] = int(m.group(2))
    assert len(blocks) == 1 and "estimation_rows_kernel" in next(iter(blocks)), sorted(blocks)
    r = next(iter(blocks.values()))
    print(r)
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r

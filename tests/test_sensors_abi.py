"""CPU side of the sensors inside the one-call collectors (include/lgsensors.h); names, exports, declarations and struct layouts:
tests/test_abi_units.py.  Here: the unit's four structs by name; one refused call per entry point that can fail leaves a message that starts with
that entry point's name; the Python surface is there and the runner's `sensor_collection` resolves to "host" without the key; the unit's one
kernel (cross-compiled for gfx950) shows no spills, no scratch and no LDS.  No GPU needed."""
import ctypes as C
import inspect
import os

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, ROOT, check_refusals, kernel_metadata, library, unit_structs


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  What the header defines."""
    assert sorted(unit_structs("sensors")) == ["lg_estimation_nets", "lg_estimation_out", "lg_sensor_camera", "lg_sensor_raycaster"]


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "runner", "sensors")
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
    check_refusals("sensors", lib, calls, quiet=quiet, returns_handle={"lg_sensor_rig_create"})
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
def test_gather_kernel_does_not_spill_and_uses_no_lds():
    """csrc/lg_sensors.hip: one kernel, the row gather, and nothing else."""
    blocks = kernel_metadata("lg_sensors.hip")
    assert len(blocks) == 1 and "estimation_rows_kernel" in next(iter(blocks)), sorted(blocks)
    r = next(iter(blocks.values()))
    print(r)
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r

"""CPU side of the terrain-estimator runner (include/lgrunner_estimator.h, `rl.NativeTerrainEstimatorRunner`, the two `terrain_est_*` scripts);
names, exports, declarations and struct layouts: tests/test_abi_units.py.  Here: the unit's structs by name; one refused call per entry point leaves
a message that starts with that entry point's name, and each refusal of the driver names its reason; the error kernel and its finish (cross-compiled
for gfx950) show no spills, no scratch and LDS within the 80 KB of the other policy-side units; the checkpoint layout against the fixture recorded
from the reference's module (tests/golden/estimator_runner_layout.json, tools/refgen/make_estimator_runner_golden.py); the Python refusals; the
scripts' `--help` and the reference's `train_cfg` from default arguments.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, ROOT, check_no_spill_no_scratch, check_refusals, kernel_metadata, last_error, library, unit_structs

LDS_SHARED = 80 * 1024
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "estimator_runner_layout.json")))


def test_structs_and_python_surface():
    assert sorted(unit_structs("runner_estimator")) == ["lg_estimation_driver", "lg_estimation_stats"]
    from extended_legged_gym_amd import rl
    assert all(hasattr(rl, n) for n in ("NativeTerrainEstimatorRunner", "collect_estimation_driven", "estimation_errors", "TerrainEstimatorTorch"))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_estimator
    assert train_estimator.TerrainEstimatorTorch is rl.TerrainEstimatorTorch          # the tool imports the class back from the package


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "runner", "sensors", "runner_estimator")
    p = 0x1000          # never read: the NULL handle / the bad argument is refused first
    est = abi.lg_estimation_out(*[p] * 5)
    stats = abi.lg_estimation_stats(*[p] * 7, 1 << 20)
    drv = abi.lg_estimation_driver(actor=p)
    calls = {
        "lg_estimation_errors": lambda: lib.lg_estimation_errors(None, p, 1, 4, 8, C.byref(stats), None),
        "lg_runner_collect_estimation": lambda: lib.lg_runner_collect_estimation(None, C.byref(drv), 4, C.byref(est), None, None, None),
    }
    check_refusals("runner_estimator", lib, calls, quiet={"lg_estimation_errors_workspace"})
    # the size function says a negative count for a bad shape, and 4 R floats per slab of four rows, 128 slabs at most
    assert lib.lg_estimation_errors_workspace(0, 8) < 0 and lib.lg_estimation_errors_workspace(4, 0) < 0 and lib.lg_estimation_errors_workspace(4, 65537) < 0
    assert lib.lg_estimation_errors_workspace(3, 25) == 100 and lib.lg_estimation_errors_workspace(33, 512) == 9 * 4 * 512
    assert lib.lg_estimation_errors_workspace(4096, 512) == 128 * 4 * 512
    # the driver's refusals, each by name, before the rig is looked at
    for field, word in (("critic", "critic"), ("std", "sampling"), ("privileged_observations", "two observation streams")):
        bad = abi.lg_estimation_driver(actor=p, **{field: p})
        assert lib.lg_runner_collect_estimation(None, C.byref(bad), 4, C.byref(est), None, None, None) == abi.LG_ERR_INVALID
        assert last_error(lib).startswith("lg_runner_collect_estimation: ") and word in last_error(lib), last_error(lib)
    bad = abi.lg_estimation_driver(actor=p, normalizer=p, normalizer_training=1)
    assert lib.lg_runner_collect_estimation(None, C.byref(bad), 4, C.byref(est), None, None, None) == abi.LG_ERR_INVALID and "training mode" in last_error(lib)
    assert lib.lg_runner_collect_estimation(None, None, 4, C.byref(est), None, None, None) == abi.LG_ERR_INVALID and "null driver" in last_error(lib)
    # the error figures: shapes, a NULL member, a short workspace
    assert lib.lg_estimation_errors(p, p, 0, 4, 8, C.byref(stats), None) == abi.LG_ERR_INVALID and "steps" in last_error(lib)
    short = abi.lg_estimation_stats(*[p] * 7, 16)
    assert lib.lg_estimation_errors(p, p, 1, 4, 8, C.byref(short), None) == abi.LG_ERR_INVALID and "workspace holds 16 floats" in last_error(lib)
    hole = abi.lg_estimation_stats(p, None, p, p, p, p, p, 1 << 20)
    assert lib.lg_estimation_errors(p, p, 1, 4, 8, C.byref(hole), None) == abi.LG_ERR_INVALID and "null member" in last_error(lib)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_error_kernels_do_not_spill_and_fit_the_lds():
    """csrc/lg_runner_estimator.hip: the error kernel and its single-workgroup finish, nothing else."""
    blocks = kernel_metadata("lg_runner_estimator.hip")
    kernels = ("estimation_error_kernel", "estimation_error_finish_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    check_no_spill_no_scratch(blocks, kernels, LDS_SHARED)


def _optimizer_state(names_shapes, step):
    rng = np.random.default_rng(3)
    tensors = lambda: {n: torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for n, s in names_shapes}          # noqa: E731
    return dict(parameters=tensors(), exp_avg=tensors(), exp_avg_sq=tensors(), step=step, learning_rate=1e-3)


@pytest.mark.parametrize("tag", sorted(GOLDEN["checkpoint"]))
def test_checkpoint_layout_is_the_reference_modules(tag):
    """Names, shapes and order of `TerrainEstimatorTorch`'s parameters and of the optimiser dict the runner writes, against what the reference's
    `TerrainEstimator` + `torch.optim.Adam` hold; and the dict loads into torch's Adam over the restatement and comes back unchanged."""
    from extended_legged_gym_amd.rl import TerrainEstimatorTorch
    from extended_legged_gym_amd.rl.estimator_runner import _all_trained, estimator_adam_state_dict
    from extended_legged_gym_amd.rl.runner import from_adam_state_dict
    g = GOLDEN["checkpoint"][tag]
    model = TerrainEstimatorTorch(tuple(g["depth_image_shape"]), g["proprio_dim"], g["num_raycast_outputs"], **g["estimator_cfg"])
    named = [[n, list(p.shape)] for n, p in model.named_parameters()]
    assert named == g["named_parameters"] and list(model.state_dict().keys()) == g["state_dict_keys"]
    state = _optimizer_state([(n, tuple(s)) for n, s in named], step=1)
    adam = estimator_adam_state_dict(state)
    assert sorted(adam.keys()) == g["optimizer_state_keys"] and sorted(adam["state"].keys()) == g["optimizer_state_indices"]
    assert list(adam["param_groups"][0].keys()) == g["param_group_keys"] and adam["param_groups"][0]["params"] == g["params"]
    assert {k: v for k, v in adam["param_groups"][0].items() if k != "params"} == {k: (tuple(v) if isinstance(v, list) else v) for k, v in g["param_group"].items()}
    assert {k: [str(v.dtype), list(v.shape)] for k, v in adam["state"][0].items()} == g["optimizer_entry"]
    for i, (n, s) in enumerate(named):
        assert list(adam["state"][i]["exp_avg"].shape) == s and torch.equal(adam["state"][i]["exp_avg_sq"], state["exp_avg_sq"][n])
    opt = torch.optim.Adam(model.parameters(), lr=0.5)
    opt.load_state_dict(adam)
    assert opt.param_groups[0]["lr"] == 1e-3
    back = from_adam_state_dict(state["parameters"], opt.state_dict(), list, _all_trained)
    assert back["step"] == 1 and all(torch.equal(back["exp_avg"][n], state["exp_avg"][n]) for n, _ in named)
    assert estimator_adam_state_dict(_optimizer_state([(n, tuple(s)) for n, s in named], step=0))["state"] == {}          # an optimiser that has not stepped


class _NoSensors:
    num_obs, num_actions, num_envs = 48, 12, 4


def _cfg(**runner):
    from extended_legged_gym_amd.scripts.terrain_est_train import create_terrain_estimator_config, get_terrain_estimator_args
    cfg = create_terrain_estimator_config(get_terrain_estimator_args([]))
    cfg["runner"].update(runner)
    return cfg


def test_python_refusals_need_no_gpu(monkeypatch):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner, collect_estimation_driven
    with pytest.raises(ValueError, match="both the depth camera and the ray caster"):
        NativeTerrainEstimatorRunner(_NoSensors(), _cfg())
    cfg = _cfg()
    cfg["algorithm"]["multi_gpu_cfg"] = {"world_size": 2}
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeTerrainEstimatorRunner(_NoSensors(), cfg)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        NativeTerrainEstimatorRunner(_NoSensors(), _cfg())
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="exactly one of policy and actions"):
        collect_estimation_driven(_NoSensors(), 4)
    with pytest.raises(ValueError, match="give an estimator"):
        collect_estimation_driven(_NoSensors(), 4, actions=torch.zeros(4, 4, 12), stats=True)


@pytest.mark.parametrize("name", ["terrain_est_train", "terrain_est_play"])
def test_scripts_parse_help_and_build_the_references_train_cfg(name, capsys):
    import importlib
    mod = importlib.import_module("extended_legged_gym_amd.scripts." + name)
    get_args = mod.get_terrain_estimator_args if name == "terrain_est_train" else mod.get_terrain_estimator_play_args
    with pytest.raises(SystemExit) as stop:
        get_args(["--help"])
    assert stop.value.code == 0
    text = capsys.readouterr().out
    assert all(flag in text for flag in ("--pretrained_policy", "--load_run", "--checkpoint", "--resume", "--task"))
    args = get_args([])
    assert mod.create_terrain_estimator_config(args) == GOLDEN["train_cfg"]
    assert args.task == "elspider_air_rough_raycast"          # the one default that differs: the reference's names a task its registry does not hold
    recorded = GOLDEN["train_defaults" if name == "terrain_est_train" else "play_defaults"]
    assert {k: getattr(args, k) for k in recorded if k != "task"} == {k: v for k, v in recorded.items() if k != "task"}
    assert callable(mod.setup_environment_for_terrain_estimation)
    # this project's two keys enter the runner block only when given
    got = mod.create_terrain_estimator_config(get_args(["--sensor_collection", "native", "--encoder_precision", "bf16"]))["runner"]
    assert got["sensor_collection"] == "native" and got["encoder_precision"] == "bf16"


def test_first_run_creates_the_experiment_directory(tmp_path, monkeypatch):
    """`find_checkpoint` and the directory logic of the train script, without an env: the newest `estimator_<it>.pt`, None for an empty run."""
    from extended_legged_gym_amd.scripts.terrain_est_train import experiment_name_of, find_checkpoint, get_terrain_estimator_args
    args = get_terrain_estimator_args([])
    assert experiment_name_of(args) == "terrain_estimator_elspider_air_rough_raycast"
    run = tmp_path / "run"
    run.mkdir()
    assert find_checkpoint(str(run)) is None
    for it in (0, 100, 20):
        (run / f"estimator_{it}.pt").write_bytes(b"")
    assert find_checkpoint(str(run)).endswith("estimator_100.pt") and find_checkpoint(str(run), 20).endswith("estimator_20.pt")

"""Golden data for the native terrain-estimator runner: the reference's `TerrainEstimator` with `torch.optim.Adam`, and the `train_cfg` its
training script builds from default arguments, run in the build container on torch-CPU.  BUILD-CONTAINER ONLY, like its neighbours.

tests/golden/estimator_runner_layout.json:
  checkpoint        for the script's estimator (GRU) and an LSTM variant: the ordered (name, shape) list of `named_parameters()`, the keys of
                    `state_dict()`, and the key lists / one entry / the parameter group of `optimizer.state_dict()` after one step;
  train_cfg         `create_terrain_estimator_config(args)` of `legged_gym/scripts/terrain_est_train.py` for its default arguments;
  train_defaults / play_defaults      name -> default of the two scripts' argument lists.
Data only: names, shapes, settings."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
from rsl_rl.modules import TerrainEstimator  # noqa: E402


def defaults_of(get_args):
    """Runs a script's argument function with `gymutil.parse_arguments` replaced by a plain argparse over its own parameter list, no command line."""
    seen = {}

    def parse_arguments(description="", custom_parameters=()):
        parser = argparse.ArgumentParser(description=description)
        for param in custom_parameters:
            parser.add_argument(param["name"], **{k: v for k, v in param.items() if k != "name"})
        args = parser.parse_args([])
        seen.update(vars(args))
        return args
    sys.modules["isaacgym.gymutil"].parse_arguments = parse_arguments
    return get_args(), dict(seen)


layout = {"checkpoint": {}}
est_cfg = dict(encoder_output_dim=64, memory_hidden_size=256, memory_num_layers=1, memory_type="gru", decoder_hidden_dims=[128, 64], activation="elu")
for tag, extra in (("gru", {}), ("lstm_2", dict(memory_type="lstm", memory_num_layers=2, memory_hidden_size=48, decoder_hidden_dims=[40]))):
    cfg = dict(est_cfg, **extra)
    torch.manual_seed(0)
    est = TerrainEstimator(depth_image_shape=(28, 56), proprio_dim=6, num_raycast_outputs=25, **cfg)
    opt = torch.optim.Adam(est.parameters(), lr=1e-3)
    sum((p ** 2).sum() for p in est.parameters()).backward()
    opt.step()
    osd = opt.state_dict()
    layout["checkpoint"][tag] = dict(
        estimator_cfg=cfg, depth_image_shape=[28, 56], proprio_dim=6, num_raycast_outputs=25,
        named_parameters=[[n, list(p.shape)] for n, p in est.named_parameters()], state_dict_keys=list(est.state_dict().keys()),
        optimizer_state_keys=sorted(osd.keys()), optimizer_state_indices=sorted(osd["state"].keys()),
        optimizer_entry={k: [str(v.dtype), list(v.shape)] for k, v in osd["state"][0].items()},
        param_group={k: v for k, v in osd["param_groups"][0].items() if k != "params"}, param_group_keys=list(osd["param_groups"][0].keys()),
        params=list(osd["param_groups"][0]["params"]))

from legged_gym.scripts import terrain_est_train, terrain_est_play  # noqa: E402

args, layout["train_defaults"] = defaults_of(terrain_est_train.get_terrain_estimator_args)
layout["train_cfg"] = terrain_est_train.create_terrain_estimator_config(args)
_, layout["play_defaults"] = defaults_of(terrain_est_play.get_terrain_estimator_play_args)

path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "estimator_runner_layout.json")
with open(path, "w") as f:
    json.dump(layout, f, indent=1, sort_keys=True)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")

"""The torch restatement of the reference's `TerrainEstimator` in `tools/train_estimator.py`, loaded with the closed-form weights, against the
outputs recorded from the reference's own module (tests/golden/terrain_estimator.npz, `tools/refgen/make_estimator_golden.py`): predictions and
hidden states of six consecutive steps with resets in between, for every case.  This pins our module -- pooling windows, flatten order, reset
semantics, key names -- to the reference's.  Bar: max(2e-5, 4 x the case's own recorded fp32-vs-float64 gap).  Also the loading rules of
`NativeTerrainEstimator` as far as they run without a device (`parse_estimator_state`).  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from train_estimator import GOLDEN_CASES, TerrainEstimatorTorch, closed_form_depth, closed_form_state  # noqa: E402

from extended_legged_gym_amd.rl.estimator import parse_estimator_state  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "terrain_estimator.npz"))
T, N, P, R = 6, 8, 6, 81


def golden_module(case, dtype=torch.float32):
    name, shape, mem, act = case
    m = TerrainEstimatorTorch(shape, P, R, memory_type=mem, activation=act)
    m.load_state_dict(closed_form_state(m, salt=GOLDEN_CASES.index(case)))
    return m.to(dtype)


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "terrain_estimator.npz")) < 1274873
    for name, shape, mem, _ in GOLDEN_CASES:
        assert G[name + "/predictions"].shape == (T, N, R) and G[name + "/proprio"].shape == (T, N, P) and G[name + "/dones"].shape == (T, N)
        assert G[name + "/hidden"].shape == (T, 2 if mem == "lstm" else 1, 1, N, 256)
        assert G[name + "/dones"].sum() == 5 and (G[name + "/gap"] > 0).all() and (G[name + "/gap"] < 5e-6).all()


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_torch_restatement_reproduces_the_reference(case):
    name, shape = case[0], case[1]
    m = golden_module(case)
    depth = closed_form_depth(T, N, *shape)
    proprio, dones = torch.from_numpy(G[name + "/proprio"]), torch.from_numpy(G[name + "/dones"])
    bar_p, bar_h = (max(2e-5, 4.0 * g) for g in G[name + "/gap"])
    with torch.no_grad():
        for t in range(T):
            pred = m.act_inference(depth[t], proprio[t])
            h = m.get_hidden_states()
            h = torch.stack(list(h) if isinstance(h, tuple) else [h])
            err_p = float((pred - torch.from_numpy(G[name + "/predictions"][t])).abs().max())
            err_h = float((h - torch.from_numpy(G[name + "/hidden"][t])).abs().max())
            print(f"{name} step {t}: predictions err {err_p:.3e} (gap {G[name + '/gap'][0]:.3e}, bar {bar_p:.3e}); hidden err {err_h:.3e} (bar {bar_h:.3e})")
            assert err_p <= bar_p and err_h <= bar_h, (name, t, err_p, err_h)
            m.reset(dones[t])
    # the rows reset after step 1 differ from a run that never resets: the fixture exercises the reset
    assert float(np.abs(G[name + "/hidden"][2][..., [0, 5], :]).max()) > 0


def test_pooling_windows_and_flatten_order():
    """torch's adaptive windows [floor(i L / 4), ceil((i + 1) L / 4)) on the 4 x 7 map of a 28 x 56 image, channel-major flatten: the layout the
    pooling kernel writes."""
    x = torch.arange(2 * 4 * 7, dtype=torch.float32).reshape(1, 2, 4, 7)
    y = torch.nn.Flatten()(torch.nn.AdaptiveAvgPool2d((4, 4))(x))[0]
    for c in range(2):
        for i in range(4):
            for j, (x0, x1) in enumerate(((0, 2), (1, 4), (3, 6), (5, 7))):
                assert y[c * 16 + i * 4 + j] == x[0, c, i, x0:x1].mean()


def test_loading_rules_without_a_device():
    m = TerrainEstimatorTorch((28, 56), 6, 187, encoder_output_dim=48, memory_hidden_size=96, memory_num_layers=2, memory_type="lstm", decoder_hidden_dims=(80, 40, 24))
    sd = m.state_dict()
    assert sorted({k.split(".")[1] for k in sd if k.startswith("depth_encoder.")}, key=int) == ["0", "2", "4", "6", "10", "12"]
    spec = parse_estimator_state(sd, (28, 56), 6, "lstm")
    assert (spec["encoder_output_dim"], spec["memory_hidden_size"], spec["memory_num_layers"], spec["decoder_hidden_dims"], spec["num_raycast_outputs"]) == \
        (48, 96, 2, [80, 40, 24], 187)
    assert len(spec["encoder"]) == 6 and spec["encoder"][4][0].shape == (128, 1024) and spec["combine"][0].shape == (48, 54)
    # a runner file (model_state_dict inside) loads the same
    assert parse_estimator_state({"model_state_dict": sd, "iter": 3}, (28, 56), 6, "lstm")["num_raycast_outputs"] == 187
    for kwargs, key in ((dict(proprio_dim=9), "combination_mlp.0.weight"), (dict(memory_type="gru"), "memory.rnn.weight_hh_l0")):
        args = dict(depth_image_shape=(28, 56), proprio_dim=6, memory_type="lstm")
        args.update(kwargs)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            parse_estimator_state(sd, **args)
    bad = dict(sd)
    bad["depth_encoder.4.weight"] = torch.zeros(128, 64, 5, 5)
    with pytest.raises(ValueError, match=r"depth_encoder\.4\.weight"):
        parse_estimator_state(bad, (28, 56), 6, "lstm")
    bad = dict(sd)
    bad["decoder.2.weight"] = torch.zeros(40, 81)
    with pytest.raises(ValueError, match=r"decoder\.2\.weight"):
        parse_estimator_state(bad, (28, 56), 6, "lstm")
    with pytest.raises(ValueError, match="depth_image_shape"):
        parse_estimator_state(sd, (200, 56), 6, "lstm")
    with pytest.raises(KeyError):
        parse_estimator_state({k: v for k, v in sd.items() if not k.startswith("memory.")}, (28, 56), 6, "lstm")

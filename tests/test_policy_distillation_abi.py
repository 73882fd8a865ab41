"""CPU side of the distillation path (include/lgpolicy.h: `lg_obs_history_step`, `lg_distill_act*`, `lg_collect_distillation*`): the built library
exports and declares every new entry point, the two new structs have the header's layout, bad shapes are refused with a status and a message, the new
kernels' code-object metadata shows no scratch and no spills while the existing kernels keep their numbers, and the golden file agrees with a numpy
forward through its own weights.  No GPU needed.  (A width mismatch between two networks needs two `lg_mlp` handles, which exist only on a device:
those refusals are in tests/test_hip_distillation.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from oracle import policy_oracle
from tests.abi_checks import HIPCC, ROOT, kernel, kernel_metadata, last_error, library

NEW = ["lg_obs_history_step", "lg_distill_act", "lg_distill_act_recurrent", "lg_collect_distillation", "lg_collect_distillation_recurrent"]
G = np.load(os.path.join(ROOT, "tests", "golden", "policy_distillation.npz"))


def _lib():
    return library("policy")


def test_new_symbols_are_exported_and_declared():
    lib = _lib()
    for sym in NEW:
        assert sym in abi.POLICY_SYMBOLS and hasattr(lib, sym), sym
    for sym in NEW:
        assert getattr(lib, sym).argtypes, sym
    from extended_legged_gym_amd import rl
    for name in ("NativeStudentTeacher", "NativeStudentTeacherRecurrent", "collect_distillation"):
        assert hasattr(rl, name), name


def test_struct_layouts_match_the_header():
    """(The layouts: tests/test_abi_units.py.)  Seven row pointers, nothing else."""
    assert C.sizeof(abi.lg_distill_rollout) == 7 * C.sizeof(C.c_void_p)


def test_obs_history_step_refuses_bad_shapes_with_a_message():
    lib = _lib()
    p = 0x1000                # never dereferenced: the shapes are refused before anything touches a pointer
    inf = float("inf")

    def call(history=p, n=8, H=3, W=48, obs=p, stride=235, clip=inf):
        return lib.lg_obs_history_step(history, n, H, W, obs, stride, None, None, None, 0, 0, clip, None, None)
    for kwargs, word in ((dict(H=0), "H"), (dict(W=0), "W"), (dict(stride=47), "stride"), (dict(clip=0.0), "clip"), (dict(clip=-1.0), "clip"),
                         (dict(history=None), "null"), (dict(obs=None), "null")):
        assert call(**kwargs) == abi.LG_ERR_INVALID, kwargs
        msg = last_error(lib)
        assert "lg_obs_history_step" in msg and word in msg, (kwargs, msg)
    assert call(n=0) == abi.LG_OK             # nothing to do, nothing launched


def test_distill_entry_points_refuse_missing_networks_with_a_message():
    lib = _lib()
    p = 0x1000
    assert lib.lg_distill_act(None, None, p, p, 4, p, 0, 0, 0, p, p, p, None) == abi.LG_ERR_INVALID
    assert "lg_distill_act" in last_error(lib)
    assert lib.lg_distill_act_recurrent(None, None, None, None, p, p, 4, p, 0, 0, 0, p, p, p, p, None, p, p, p, None) == abi.LG_ERR_INVALID
    assert "lg_distill_act_recurrent" in last_error(lib)
    rows = abi.lg_distill_rollout()
    assert lib.lg_collect_distillation(None, None, None, p, 0, 0, 24, None, C.byref(rows), None) == abi.LG_ERR_INVALID
    assert "lg_collect_distillation" in last_error(lib)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch_and_the_existing_ones_keep_their_numbers():
    blocks = kernel_metadata("lg_policy.hip")

    def one(part):
        return kernel(blocks, part)
    for part in ("obs_history_kernel", "obs_clip_kernel", "distill_act_kernel"):
        r = one(part)
        print(part, r)
        assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (part, r)
    assert one("obs_history_kernel")["group_segment_fixed_size"] == 0
    # the added instance of the PPO.act body drops the log-prob rows (32 x 32 floats) and nothing else
    act, dist = one("policy_act_kernel"), one("distill_act_kernel")
    assert act["group_segment_fixed_size"] == 139264 and dist["group_segment_fixed_size"] == 139264 - 32 * 32 * 4
    assert act["vgpr_count"] == 140 and dist["vgpr_count"] <= 140 and act["private_segment_fixed_size"] == 0
    rnn = one("rnn_layer_kernel")
    assert rnn["vgpr_count"] == 113 and rnn["group_segment_fixed_size"] == 131072 and rnn["private_segment_fixed_size"] == 0
    assert one("mlp_forward_kernel")["vgpr_count"] == 124 and one("mlp_forward_kernel")["group_segment_fixed_size"] == 131072


@pytest.mark.parametrize("case", ["ff", "lstm", "gru", "lstm_tr", "gru_tr"])
def test_golden_outputs_agree_with_a_numpy_forward(case):
    """Guards the fixture: the recorded float32 outputs of every MLP whose input is in the file (the feed-forward student, a teacher without a memory)
    against `oracle/policy_oracle.py` in float64 through the stored weights, at the bar of the GPU test: max(2e-5, 4 x the recorded fp32-vs-float64 gap)."""
    pre = case + ".sd."
    sd = {k[len(pre):]: G[k].astype(np.float32) for k in G.files if k.startswith(pre)}
    assert sd["std"].shape == (12,) and all(np.isfinite(v).all() for v in sd.values())
    assert ("memory_s.rnn.weight_ih_l0" in sd) == (case != "ff") and ("memory_t.rnn.weight_ih_l0" in sd) == case.endswith("_tr")
    bar = np.maximum(2e-5, 4.0 * G[case + ".fp32_vs_fp64_maxabs"])
    T = G["obs"].shape[0]
    assert bar.shape == (T,) and G[case + ".action_mean"].shape == G[case + ".privileged_actions"].shape == (T, 7, 12)
    checks = []
    if case == "ff":
        checks.append(("student", G["obs"], case + ".action_mean"))
    if not case.endswith("_tr"):
        checks.append(("teacher", G["tobs"], case + ".privileged_actions"))
    for prefix, x, key in checks:
        layers = policy_oracle.sequential_layers(sd, prefix)
        for t in range(T):
            err = np.abs(policy_oracle.mlp_forward(layers, x[t]) - G[key][t]).max()
            assert err <= bar[t], (prefix, t, err, bar[t])
    if case != "ff":
        h = G[case + ".h_s"]
        assert h.shape == (T, 2, 7, 40) and np.abs(h).max() <= 1.0
        # the dones of a step zero the rows AFTER that step's act: the recorded state of the step still holds them
        assert all(np.abs(h[t][:, G["dones"][t] == 1]).max() > 0 for t in G["meta.reset_steps"])
    else:
        assert abs(G["ff.update_loss"] - G["ff.update_per_batch"].mean()) <= 1e-12 and G["ff.update_per_batch"].shape == (T,)


def test_tool_update_reproduces_the_reference_behaviour_loss():
    """`tools/train_distill.py`'s restatement of `Distillation.update` on the golden rows, from the golden weights, on the CPU: the mean behaviour loss
    and every per-batch loss the reference recorded (one Adam step after batch 15 included).  Bar: 4 x the yardstick the generator records -- the
    largest |float32 - float64| over the reference's own per-batch losses -- the project's factor for a float32 result against its float64 twin; a
    mean of T N A = 2016 squared terms of O(0.1) rounds well inside it."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from train_distill import StudentTeacher, distill_update
    pre = "ff.sd."
    sd = {k[len(pre):]: torch.from_numpy(G[k].astype(np.float32)) for k in G.files if k.startswith(pre)}
    policy = StudentTeacher(20, 24, 12, [32, 16], [32, 16], 0.1)
    policy.load_state_dict(sd)
    rows = {"observations": torch.from_numpy(G["obs"]), "privileged_actions": torch.from_numpy(G["ff.privileged_actions"])}
    per_batch = []
    inner = torch.nn.functional.mse_loss
    torch.nn.functional.mse_loss = lambda a, b: (lambda l: (per_batch.append(float(l.item())), l)[1])(inner(a, b))
    try:
        loss = distill_update(policy, torch.optim.Adam(policy.parameters(), lr=1e-3), rows, gradient_length=15, max_grad_norm=1.0)
    finally:
        torch.nn.functional.mse_loss = inner
    yard = float(np.abs(G["ff.update_per_batch"] - G["ff.update_per_batch_fp64"]).max())
    bar = 4.0 * yard
    err = abs(loss - float(G["ff.update_loss"]))
    worst = float(np.abs(np.array(per_batch) - G["ff.update_per_batch"]).max())
    print(f"behaviour loss {loss:.9g} (reference {float(G['ff.update_loss']):.9g}): |diff| {err:.3e}, per batch {worst:.3e}; yardstick {yard:.3e}, bar {bar:.3e}")
    assert yard > 0 and err <= bar and worst <= bar
    assert not torch.equal(policy.student[0].weight, sd["student.0.weight"]) and torch.equal(policy.teacher[0].weight, sd["teacher.0.weight"])

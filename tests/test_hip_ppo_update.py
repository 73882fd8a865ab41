"""The native PPO update (include/lgtrain.h, `rl.NativePPO`) on the GPU against tests/ppo_reference.py in float64.

The bar of the gradient checks is measured, not guessed: torch's own fp32 CPU autograd on the same inputs deviates from float64 by e32(t) per tensor
(e(t) = max|t - t64| / max|t64|); the kernels may deviate by at most max(8 e32(t), 2e-5) -- 8 for a different summation order over the batch and
`apply_act`'s ELU polynomial, 2e-5 the project's forward tolerance.  Every figure is printed before it is asserted.

Shapes: S1 the "odd" golden network (widths off the 16 grid, separate critic observations) on a ragged 32-row tile; S2 two full weight-gradient
slabs and a ragged third (ELU, ReLU, SELU); S3 one-layer networks (no activation, no backward data pass); S4 the "rough" golden network (the widest
layer, the LDS limit)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ppo_reference as ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def _slab():
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl.ppo import _train_lib
    assert abi.TRAIN_SYMBOLS
    return int(_train_lib().lg_ppo_wgrad_slab_rows())


def _golden_sd(name):
    z = np.load(os.path.join(GOLD, "policy.npz"))
    pre = name + ".sd."
    return {k[len(pre):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(pre)}


def _random_sd(actor_dims, critic_dims, seed, std=0.7):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for prefix, dims in (("actor", actor_dims), ("critic", critic_dims)):
        for j in range(len(dims) - 1):
            bound = 1.0 / np.sqrt(dims[j])
            sd[f"{prefix}.{2 * j}.weight"] = (torch.rand(dims[j + 1], dims[j], generator=g) * 2 - 1) * bound * 1.7
            sd[f"{prefix}.{2 * j}.bias"] = (torch.rand(dims[j + 1], generator=g) * 2 - 1) * bound
    sd["std"] = std * (1.0 + 0.2 * torch.rand(actor_dims[-1], generator=g))
    return sd


def _case(shape, std_type):
    """(state dict, activation, rows per mini-batch)."""
    if shape == "S1":
        sd, act, n = _golden_sd("odd"), "tanh", 37
    elif shape.startswith("S2"):
        sd, act, n = _random_sd([48, 64, 32, 12], [48, 64, 32, 1], 3), shape.split("-")[1], 2 * _slab() + 13
    elif shape == "S3":
        sd, act, n = _random_sd([5, 3], [5, 1], 4), "elu", 37
    else:
        sd, act, n = _golden_sd("rough"), "elu", 96
    if std_type == "log":
        sd = dict(sd)
        sd["log_std"] = torch.log(sd.pop("std"))
    return sd, act, n


def _build(sd, act, std_type, max_rows=None, **kw):
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    policy = NativeActorCritic(sd, act, noise_std_type=std_type, device=DEV, seed=1)
    return policy, NativePPO(policy, sd, max_rows=max_rows, **kw)


def _cuda(rows):
    return {k: v.to(DEV) for k, v in rows.items()}


def _err(got, want):
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _within(name, e, e32):
    bar = max(8.0 * e32, 2e-5)
    print(f"{name}: e {e:.3e}  e32 {e32:.3e}  e/e32 {e / max(e32, 1e-300):.2f}  bar {bar:.3e}")
    return e <= bar


GRAD_CASES = [("S1", "scalar", True), ("S1", "log", False), ("S2-elu", "scalar", True), ("S2-relu", "log", True), ("S2-selu", "scalar", False),
              ("S3", "scalar", True), ("S3", "log", False), ("S4", "scalar", True), ("S4", "log", False)]


@pytest.mark.parametrize("shape,std_type,clipped", GRAD_CASES)
def test_gradients_losses_and_norm_against_float64(shape, std_type, clipped):
    sd, act, n = _case(shape, std_type)
    hyper = dict(ref.HYPER, use_clipped_value_loss=clipped, entropy_coef=0.01, value_loss_coef=0.8)
    rows = ref.craft_rows(sd, act, n + 19, seed=11, share_observations=shape != "S1")
    idx = torch.randperm(n + 19, generator=torch.Generator().manual_seed(5))[:n]
    policy, ppo = _build(sd, act, std_type, **{k: hyper[k] for k in hyper})
    ppo.minibatch(_cuda(rows), idx)
    g, norm, means = ppo.gradients()
    batch = ref.take(rows, idx)
    g64, n64, m64, ratio, dv = ref.gradients(sd, act, batch, hyper, torch.float64)
    g32, n32, m32, _, _ = ref.gradients(sd, act, batch, hyper, torch.float32)
    # the crafted rows populate the branches this check is about
    frac = ref.branch_fractions(ratio, dv, batch["advantages"].squeeze(-1).double(), hyper["clip_param"])
    print(shape, std_type, clipped, frac)
    assert min(frac[k] for k in frac if k.startswith(("pos", "neg"))) >= 0.05 and min(frac["value_below"], frac["value_above"]) >= 0.10, frac
    ok = True
    for k in g64:
        ok &= _within(f"{shape} {k}", _err(g[k], g64[k]), _err(g32[k], g64[k]))
    ok &= _within(f"{shape} norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for k in ("surrogate", "value_function", "entropy", "kl"):
        ok &= _within(f"{shape} {k}", abs(means[k] - float(m64[k])) / abs(float(m64[k])), abs(float(m32[k]) - float(m64[k])) / abs(float(m64[k])))
    assert ok


def _ulp(t):
    t = t.double().abs()
    return torch.where(t > 0, 2.0 ** (torch.floor(torch.log2(t.clamp_min(1e-300))) - 23), torch.full_like(t, 2.0 ** -149))


@pytest.mark.parametrize("max_grad_norm", [0.05, 1.0e3])
def test_optimiser_step_on_the_kernels_own_gradients(max_grad_norm):
    sd, act, n = _case("S1", "scalar")
    hyper = dict(ref.HYPER, max_grad_norm=max_grad_norm, entropy_coef=0.01)
    rows = ref.craft_rows(sd, act, n, seed=12)
    lr = 2.5e-3
    policy, ppo = _build(sd, act, "scalar", learning_rate=lr, **hyper)
    g = torch.Generator().manual_seed(8)
    state = dict(parameters=sd, exp_avg={k: 0.01 * torch.randn(v.shape, generator=g) for k, v in sd.items()},
                 exp_avg_sq={k: 1e-4 * torch.rand(v.shape, generator=g) for k, v in sd.items()}, step=7, learning_rate=lr)
    ppo.load_optimizer_state(state)
    back = ppo.optimizer_state()
    assert back["step"] == 7 and back["learning_rate"] == lr
    for k in sd:
        assert torch.equal(back["exp_avg"][k], state["exp_avg"][k]) and torch.equal(back["parameters"][k], sd[k]), k
        assert torch.equal(back["exp_avg_sq"][k], state["exp_avg_sq"][k]), k
    ppo.minibatch(_cuda(rows), torch.arange(n))
    grads, norm, _ = ppo.gradients()
    print("norm", norm, "max_grad_norm", max_grad_norm)
    assert (norm > max_grad_norm) == (max_grad_norm < 1.0)          # the clip bites in one case and not in the other
    want, wstate = ref.clip_and_adam(sd, grads, dict(exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"], step=7), lr, max_grad_norm)
    after = ppo.optimizer_state()
    assert after["step"] == 8
    worst = 0.0
    for k in sd:
        tol = 1e-5 * lr + _ulp(want[k])
        excess = ((after["parameters"][k].double() - want[k]).abs() / tol).max()
        worst = max(worst, float(excess))
        for moment in ("exp_avg", "exp_avg_sq"):          # a few fp32 roundings of numbers no larger than the tensor's largest
            assert float((after[moment][k].double() - wstate[moment][k]).abs().max()) <= 1e-6 * float(wstate[moment][k].abs().max()) + 1e-12, (moment, k)
    print("largest |theta - theta64| / (1e-5 lr + 1 ulp):", worst)
    assert worst <= 1.0


def test_learning_rate_rule_on_each_side_of_both_thresholds():
    sd, act, n = _case("S3", "scalar")
    rows = ref.craft_rows(sd, act, n, seed=13, share_observations=True)
    _, _, m64, _, _ = ref.gradients(sd, act, rows, ref.HYPER, torch.float64)
    kl, lr = float(m64["kl"]), 1e-3
    assert kl > 0
    for desired, want in ((kl / 2 / 1.25, max(1e-5, lr / 1.5)), (kl / 2 * 1.25, lr), (2 * kl / 1.25, lr), (2 * kl * 1.25, min(1e-2, lr * 1.5))):
        policy, ppo = _build(sd, act, "scalar", learning_rate=lr, **dict(ref.HYPER, schedule="adaptive", desired_kl=desired))
        ppo.minibatch(_cuda(rows), torch.arange(n))
        got = ppo.optimizer_state()["learning_rate"]
        print("kl", kl, "desired_kl", desired, "lr", got)
        assert got == want
    policy, ppo = _build(sd, act, "scalar", learning_rate=lr, **dict(ref.HYPER, schedule="fixed", desired_kl=2 * kl * 1.25))
    ppo.minibatch(_cuda(rows), torch.arange(n))
    assert ppo.optimizer_state()["learning_rate"] == lr


@pytest.mark.parametrize("shape,std_type", [("S1", "log"), ("S2-elu", "scalar"), ("S4", "scalar")])
def test_policy_and_trainer_stay_coherent(shape, std_type):
    from extended_legged_gym_amd.rl import NativeActorCritic
    sd, act, n = _case(shape, std_type)
    rows = _cuda(ref.craft_rows(sd, act, n, seed=14, share_observations=shape != "S1"))
    policy, ppo = _build(sd, act, std_type, learning_rate=3e-3, **ref.HYPER)
    before, value_before = policy.act_inference(rows["observations"]).clone(), policy.evaluate(rows["critic_observations"]).clone()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    ppo.minibatch(rows, idx)
    # the trainer's forward pass (gathered rows, saved activations) computes lg_mlp_forward's values bit for bit
    mu, val = ppo.forward_outputs(n)
    assert torch.equal(mu, before.cpu()[idx]) and torch.equal(val, value_before.cpu()[idx])
    ppo.minibatch(rows, torch.arange(n - 5))
    new_sd = ppo.state_dict()
    fresh = NativeActorCritic(new_sd, act, noise_std_type=std_type, device=DEV, seed=1)
    a, b = policy.act_inference(rows["observations"]), fresh.act_inference(rows["observations"])
    assert torch.equal(a, b) and not torch.equal(a, before)
    assert torch.equal(policy.evaluate(rows["critic_observations"]), fresh.evaluate(rows["critic_observations"]))
    want_std = new_sd["std"] if std_type == "scalar" else torch.exp(new_sd["log_std"])
    if std_type == "scalar":
        assert torch.equal(policy.std.cpu(), want_std)
    else:                                                       # expf on the device against torch's exp: a rounding or two
        assert torch.allclose(policy.std.cpu(), want_std, rtol=3e-7, atol=0)


def _state_equal(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


def test_one_update_call_equals_the_loop_and_is_deterministic():
    sd, act, _ = _case("S1", "scalar")
    R, E, M = 3 * 50 + 2, 2, 3
    rows = _cuda(ref.craft_rows(sd, act, R, seed=15, kl_scale=0.02))
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3))
    kw = dict(ref.HYPER, schedule="adaptive", desired_kl=0.004, entropy_coef=0.005, learning_rate=4e-3, num_learning_epochs=E, num_mini_batches=M)
    _, one = _build(sd, act, "scalar", **kw)
    _, two = _build(sd, act, "scalar", **kw)
    _, loop = _build(sd, act, "scalar", **kw)
    loss1, loss2 = one.update(rows, perm), two.update(rows, perm)
    mini, sums = R // M, dict(value_function=0.0, surrogate=0.0, entropy=0.0, kl=0.0)
    for _ in range(E):
        for i in range(M):
            loop.minibatch(rows, perm[i * mini:(i + 1) * mini])
            means = loop.gradients()[2]
            for k in sums:
                sums[k] += means[k]
    s1, s2, s3 = one.optimizer_state(), two.optimizer_state(), loop.optimizer_state()
    _state_equal(s1, s2)
    _state_equal(s1, s3)
    kl = sums.pop("kl") / (E * M)
    assert loss1 == loss2 and loss1 == {k: v / (E * M) for k, v in sums.items()}, (loss1, loss2, sums)
    assert one.kl == two.kl == kl, (one.kl, two.kl, kl)
    assert one.learning_rate == two.learning_rate == s1["learning_rate"] == s3["learning_rate"] and s1["step"] == E * M


@pytest.mark.parametrize("name", ["mb1", "mb3"])
def test_the_references_own_update(name):
    """tests/golden/ppo_update.npz (the reference's `PPO.update` on torch-CPU) through `NativePPO.update` with the recorded permutation.  The learning
    rate (a float64 on the device, stepped by the reference's rule) must match exactly, at every optimiser step.  The post-update action means and
    values are held to max(8 x the fp32-vs-fp64 deviation of the restatement, 2e-5).  The three loss means cannot be equal to the last bit: each is
    an fp32 mean over the mini-batch summed in block order here and pairwise in torch (DESIGN.md s11b gives the measured differences, 1 to 4 ulp);
    they are held to the same bar, against float64 and against the reference's recorded values."""
    case = ref.load_golden_case(name)
    sd, act, rows, perm, kw = case["sd0"], case["activation"], case["rows"], case["perm"], case["ppo"]
    hyper = {k: kw[k] for k in ref.HYPER}
    policy, ppo = _build(sd, act, case["noise_std_type"], **kw)
    loss = ppo.update(_cuda(rows), perm)
    print(name, "native", loss, ppo.learning_rate, "reference", case["loss"], case["learning_rate"])
    assert ppo.learning_rate == case["learning_rate"]
    _, loop = _build(sd, act, case["noise_std_type"], **kw)          # the same steps one by one: the learning rate of every optimiser step
    mini, lrs = rows["observations"].shape[0] // kw["num_mini_batches"], []
    for _ in range(kw["num_learning_epochs"]):
        for i in range(kw["num_mini_batches"]):
            loop.minibatch(_cuda(rows), perm[i * mini:(i + 1) * mini])
            lrs.append(loop.optimizer_state()["learning_rate"])
    print(name, "learning-rate trajectory", lrs)
    assert lrs == case["lr_trajectory"]
    p64, l64, lr64, _, _ = ref.update(sd, act, rows, perm, hyper, kw["num_learning_epochs"], kw["num_mini_batches"], kw["learning_rate"], torch.float64)
    p32, l32, lr32, _, _ = ref.update(sd, act, rows, perm, hyper, kw["num_learning_epochs"], kw["num_mini_batches"], kw["learning_rate"], torch.float32)
    assert lr64 == case["learning_rate"]
    ok = True
    for k in ("value_function", "surrogate", "entropy"):
        ok &= _within(f"{name} loss {k} vs float64", abs(loss[k] - l64[k]) / abs(l64[k]), abs(l32[k] - l64[k]) / abs(l64[k]))
        ok &= _within(f"{name} loss {k} vs the reference", abs(loss[k] - case["loss"][k]) / abs(case["loss"][k]), abs(l32[k] - l64[k]) / abs(l64[k]))
    obs, cobs = rows["observations"], rows["critic_observations"]
    mu64, v64 = ref.mlp(p64, "actor", obs.double(), act), ref.mlp(p64, "critic", cobs.double(), act)
    mu32, v32 = ref.mlp(p32, "actor", obs, act), ref.mlp(p32, "critic", cobs, act)
    ok &= _within(f"{name} action means", _err(policy.act_inference(obs.to(DEV)), mu64), _err(mu32, mu64))
    ok &= _within(f"{name} values", _err(policy.evaluate(cobs.to(DEV)), v64), _err(v32, v64))
    assert ok


def test_live_handle_refusals_leave_the_handles_usable():
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    sd, act, n = _case("S3", "scalar")
    rows = _cuda(ref.craft_rows(sd, act, n, seed=16, share_observations=True))
    policy, ppo = _build(sd, act, "scalar", max_rows=n - 1, **ref.HYPER)
    from extended_legged_gym_amd import abi
    r, _, keep = ppo._rows(rows)
    idx, hyper = torch.arange(n, device=DEV), ppo._hyper()
    rc = ppo.lib.lg_ppo_minibatch(ppo.handle, C.byref(r), C.c_void_p(idx.data_ptr()), n, C.byref(hyper), None)
    msg = (ppo.lib.lg_mlp_last_error(None) or b"").decode()
    assert rc == abi.LG_ERR_INVALID and msg.startswith("lg_ppo_minibatch: ") and "max_rows" in msg, (rc, msg)
    before = ppo.state_dict()
    ppo.minibatch(rows, torch.arange(n - 1))                    # a valid call on the same handle
    assert not torch.equal(before["actor.0.weight"], ppo.state_dict()["actor.0.weight"])
    two = _random_sd([5, 3], [5, 2], 4)
    wide = NativeActorCritic(two, act, device=DEV)
    with pytest.raises(RuntimeError, match="lg_ppo_create.*critic must end in 1 output"):
        NativePPO(wide, two, max_rows=n)
    assert wide.evaluate(rows["critic_observations"]).shape == (n, 2)          # the refused networks still run
    NativePPO(policy, sd, max_rows=n).minibatch(rows, torch.arange(n))


def test_out_of_scope_options_are_refused_by_name():
    from extended_legged_gym_amd.rl import NativePPO
    sd, act, _ = _case("S3", "scalar")
    policy, _ = _build(sd, act, "scalar")
    for opt in ("normalize_advantage_per_mini_batch", "rnd_cfg", "symmetry_cfg", "multi_gpu_cfg"):
        with pytest.raises(NotImplementedError, match=opt):
            NativePPO(policy, sd, **{opt: True if opt.startswith("normalize") else {"x": 1}})

    class Recurrent:
        is_recurrent = True
    with pytest.raises(NotImplementedError, match="recurrent"):
        NativePPO(Recurrent(), sd)

"""GPU: the native PPO and distillation updates (`rl.NativePPO`, `rl.NativeDistillation`) on networks whose observation row is wider than 512 columns
(`lg_mlp_create_wide`): the split-K first layer of the training forward (csrc/lg_train.hip: `ppo_wide_forward_kernel`) and the weight-gradient, reduce and
Adam passes at a wide `dI`.  Method and bar are those of tests/test_hip_ppo_update.py and tests/test_hip_distill_update.py: float64 restatements
(tests/ppo_reference.py, tests/distill_reference.py), every tensor within max(8 x e32, 2e-5), e32 = torch's own fp32 CPU autograd against float64.

Shapes: actor 578-64-32-18 with critic 578-48-1 (the raycast task's row, both networks wide, shared observations), and actor 1025-33-6 with critic
130-17-1 (three slabs, the last of one 64-block; a wide and a narrow network in one launch, separate observations).  The mini-batch is 70 rows (two
tiles and a ragged third) gathered through a shuffled index from 96.

The loss means are compared RELATIVE to their float64 value, and the surrogate mean is a sum of terms of both signs: over 70 rows of magnitude ~0.8 an
fp32 mean carries about sqrt(70) x 2^-24 x 0.8 = 4e-7 whatever the summation order, which is 4e-7 x c of the mean, c = mean |term| / |mean term|.  At
c = 85 (row seed 21 on the second shape; |mean| 0.0096) that alone is 3e-5, above the 2e-5 floor, and says nothing about the kernels.  So the rows
are a condition on the inputs, fixed from float64 alone: the first row seed from 21 upward with c <= 20, half of the c = 50 at which summation
order alone reaches the floor (21 for the first shape, c = 17; 24 for the second, c = 7.7)."""
import functools

import pytest
import torch

from tests import distill_reference as dref
from tests import ppo_reference as ref
from tests.test_hip_ppo_update import DEV, _build, _cuda, _err, _random_sd, _within

pytestmark = pytest.mark.gpu
SHAPES = {"578x578": ([578, 64, 32, 18], [578, 48, 1], True), "1025x130": ([1025, 33, 6], [130, 17, 1], False)}
ROWS, BATCH = 96, 70


HYPER = dict(ref.HYPER, entropy_coef=0.01, value_loss_coef=0.8)
MAX_CANCELLATION = 20.0


def _cancellation(sd, rows, idx):
    """mean |term| / |mean term| of the clipped surrogate over the mini-batch, in float64."""
    batch = ref.take(rows, idx)
    _, _, _, ratio, _ = ref.gradients(sd, "elu", batch, HYPER, torch.float64)
    adv = batch["advantages"].squeeze(-1).double()
    terms = torch.max(-adv * ratio, -adv * ratio.clamp(1.0 - HYPER["clip_param"], 1.0 + HYPER["clip_param"]))
    return float(terms.abs().mean() / terms.mean().abs())


@functools.lru_cache(maxsize=None)
def _case(shape):
    adims, cdims, share = SHAPES[shape]
    sd = _random_sd(adims, cdims, 40 + len(adims))
    idx = torch.randperm(ROWS, generator=torch.Generator().manual_seed(6))[:BATCH]
    for seed in range(21, 31):
        rows = ref.craft_rows(sd, "elu", ROWS, seed=seed, share_observations=share)
        c = _cancellation(sd, rows, idx)
        print(f"{shape}: row seed {seed}, cancellation of the surrogate mean {c:.1f}")
        if c <= MAX_CANCELLATION:
            return sd, rows, idx
    raise AssertionError(f"{shape}: no row seed in 21..30 gives a surrogate mean with cancellation <= {MAX_CANCELLATION}")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gradients_losses_and_norm_against_float64(shape):
    sd, rows, idx = _case(shape)
    hyper = HYPER
    policy, ppo = _build(sd, "elu", "scalar", **hyper)
    ppo.minibatch(_cuda(rows), idx)
    g, norm, means = ppo.gradients()
    batch = ref.take(rows, idx)
    g64, n64, m64, ratio, dv = ref.gradients(sd, "elu", batch, hyper, torch.float64)
    g32, n32, m32, _, _ = ref.gradients(sd, "elu", batch, hyper, torch.float32)
    frac = ref.branch_fractions(ratio, dv, batch["advantages"].squeeze(-1).double(), hyper["clip_param"])
    print(shape, frac)
    assert min(frac[k] for k in frac if k.startswith(("pos", "neg"))) >= 0.05 and min(frac["value_below"], frac["value_above"]) >= 0.10, frac
    ok = True
    for k in g64:
        ok &= _within(f"{shape} {k}", _err(g[k], g64[k]), _err(g32[k], g64[k]))
    ok &= _within(f"{shape} norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for k in ("surrogate", "value_function", "entropy", "kl"):
        ok &= _within(f"{shape} {k}", abs(means[k] - float(m64[k])) / abs(float(m64[k])), abs(float(m32[k]) - float(m64[k])) / abs(float(m64[k])))
    assert ok
    # every slab of the first layer's gradient carries signal: a slab that was never staged would leave zeros there
    for k0 in range(0, g64["actor.0.weight"].shape[1], 512):
        assert float(g["actor.0.weight"][:, k0:k0 + 512].abs().max()) > 0.0, (shape, k0)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_trainer_forward_policy_and_state_dict_stay_coherent(shape):
    from extended_legged_gym_amd.rl import NativeActorCritic
    sd, rows, idx = _case(shape)
    rows = _cuda(rows)
    policy, ppo = _build(sd, "elu", "scalar", learning_rate=3e-3, **ref.HYPER)
    before, value_before = policy.act_inference(rows["observations"]).clone(), policy.evaluate(rows["critic_observations"]).clone()
    ppo.minibatch(rows, idx)
    # the trainer's forward pass (rows gathered slab by slab, saved activations) computes lg_mlp_forward's values bit for bit
    mu, val = ppo.forward_outputs(BATCH)
    assert torch.equal(mu, before.cpu()[idx]) and torch.equal(val, value_before.cpu()[idx])
    ppo.update(rows, torch.randperm(ROWS, generator=torch.Generator().manual_seed(7)))
    ppo.update(rows, torch.randperm(ROWS, generator=torch.Generator().manual_seed(8)))
    new_sd = ppo.state_dict()
    fresh = NativeActorCritic(new_sd, "elu", noise_std_type="scalar", device=DEV, seed=1)
    a, b = policy.act_inference(rows["observations"]), fresh.act_inference(rows["observations"])
    assert torch.equal(a, b) and not torch.equal(a, before)
    assert torch.equal(policy.evaluate(rows["critic_observations"]), fresh.evaluate(rows["critic_observations"]))
    assert torch.equal(policy.std.cpu(), new_sd["std"])
    moved = (new_sd["actor.0.weight"] - sd["actor.0.weight"]).abs()
    assert float(moved[:, 512:].max()) > 0.0 and float(moved[:, :512].max()) > 0.0          # both sides of the slab edge train
    policy._call = fresh._call = 0
    fresh.seed = policy.seed
    one, two = policy.act_and_evaluate(rows["observations"], rows["critic_observations"]), fresh.act_and_evaluate(rows["observations"], rows["critic_observations"])
    assert all(torch.equal(x, y) for x, y in zip(one, two))


def test_distillation_with_a_578_wide_student_against_float64():
    from extended_legged_gym_amd.rl import NativeDistillation, NativeStudentTeacher
    T, N, G = 4, 33, 2
    sd = dref.random_student([578, 64, 18], 23, teacher_dims=[48, 8, 18])
    rows = dref.craft_rows(sd, "elu", T, N, 24)
    obs, tgt = rows["observations"], rows["privileged_actions"]
    policy = NativeStudentTeacher(sd, activation="elu", device=DEV, seed=1)
    alg = NativeDistillation(policy, sd, loss_type="mse", max_grad_norm=1.0, gradient_length=G)
    order = [(1 + s) % T for s in range(G)]
    before = policy.act_inference(obs[order].reshape(G * N, -1).to(DEV)).clone()
    alg.group(_cuda(rows), 1, G)
    assert torch.equal(alg.forward_outputs(G * N), before.cpu())
    g, norm, losses = alg.gradients()
    g64, n64, l64, _ = dref.group_gradients(sd, "elu", obs, tgt, 1, G, "mse", torch.float64)
    g32, n32, l32, _ = dref.group_gradients(sd, "elu", obs, tgt, 1, G, "mse", torch.float32)
    ok = len(losses) == G
    for k in g64:
        ok &= _within(f"distillation {k}", _err(g[k], g64[k]), _err(g32[k], g64[k]))
    ok &= _within("distillation norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for s in range(G):
        ok &= _within(f"distillation loss of step {s}", abs(losses[s] - float(l64[s])) / float(l64[s]), abs(float(l32[s]) - float(l64[s])) / float(l64[s]))
    assert ok
    loss = alg.update(_cuda(rows))          # the whole update runs: T = 4 steps in groups of 2
    assert loss["behavior"] > 0.0 and not torch.equal(policy.act_inference(obs[0].to(DEV)), before[:N])


def test_the_symmetric_update_refuses_a_wide_policy_by_name():
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeSymmetricPPO
    sd, rows, _ = _case("578x578")
    policy = NativeActorCritic(sd, "elu", device=DEV, seed=1)
    obs = rows["observations"].to(DEV)
    before = policy.act_inference(obs).clone()

    def mirror(obs=None, actions=None, env=None, obs_type="policy"):
        return (None if obs is None else torch.cat([obs, -obs])), (None if actions is None else torch.cat([actions, -actions]))
    with pytest.raises(NotImplementedError, match="578"):
        NativeSymmetricPPO(policy, sd, symmetry_cfg=dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.0, data_augmentation_func=mirror))
    assert torch.equal(policy.act_inference(obs), before)          # the refused policy still acts

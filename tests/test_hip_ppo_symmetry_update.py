"""The native PPO update with `symmetry_cfg` (include/lgtrain_symmetry.h, `rl.NativeSymmetricPPO`) on the GPU against tests/ppo_symmetry_reference.py
in float64, which calls the augmentation function itself: the probe's tables are held with the kernels.

The bar is the one of tests/test_hip_ppo_update.py, measured, not guessed: torch's own fp32 CPU autograd on the same inputs deviates from float64 by
e32(t) per tensor (e(t) = max|t - t64| / max|t64|); the kernels may deviate by at most max(8 e32(t), 2e-5).  Every figure is printed before it is
asserted.  The shapes are `ppo_symmetry_reference.gpu_case`'s; tests/test_ppo_symmetry_reference.py asserts, on the reference alone, that their
transformed rows populate every branch of the clipped losses and that a wrong action table would show at ten times the bar."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ppo_reference as ref
from tests import ppo_symmetry_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slab():
    from extended_legged_gym_amd.rl.ppo import _train_lib
    return int(_train_lib().lg_ppo_wgrad_slab_rows())


def _case(shape, std_type):
    sd, act, n, func, share = sref.gpu_case(shape, _slab())
    rows, idx = sref.gpu_rows(shape, _slab())
    if std_type == "log":
        sd = dict(sd)
        sd["log_std"] = torch.log(sd.pop("std"))
    return sd, act, n, func, rows, idx


def _sym(mode, func):
    return dict(sref.MODES[mode], data_augmentation_func=func, _env=None)


def _build(sd, act, std_type, sym, max_rows=None, **kw):
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeSymmetricPPO
    policy = NativeActorCritic(sd, act, noise_std_type=std_type, device=DEV, seed=1)
    return policy, NativeSymmetricPPO(policy, sd, symmetry_cfg=sym, max_rows=max_rows, **kw)


def _cuda(rows):
    return {k: v.to(DEV) for k, v in rows.items()}


def _err(got, want):
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _within(name, e, e32):
    bar = max(8.0 * e32, 2e-5)
    print(f"{name}: e {e:.3e}  e32 {e32:.3e}  e/e32 {e / max(e32, 1e-300):.2f}  bar {bar:.3e}")
    return e <= bar


GRAD_CASES = ([(s, m, "scalar") for s in sref.SHAPES for m in sref.MODES] + [(s, m, "log") for s in ("Y1", "Y4") for m in sref.MODES])


@pytest.mark.parametrize("shape,mode,std_type", GRAD_CASES)
def test_gradients_losses_and_norm_against_float64(shape, mode, std_type):
    sd, act, n, func, rows, idx = _case(shape, std_type)
    hyper = dict(ref.HYPER, entropy_coef=0.01, value_loss_coef=0.8)
    sym = _sym(mode, func)
    policy, ppo = _build(sd, act, std_type, sym, **hyper)
    ppo.minibatch(_cuda(rows), idx)
    g, norm, means = ppo.gradients()
    batch = ref.take(rows, idx)
    g64, n64, m64, _, _, _ = sref.gradients(sd, act, batch, hyper, sym, torch.float64)
    g32, n32, m32, _, _, _ = sref.gradients(sd, act, batch, hyper, sym, torch.float32)
    ok = True
    for k in g64:
        ok &= _within(f"{shape} {mode} {k}", _err(g[k], g64[k]), _err(g32[k], g64[k]))
    ok &= _within(f"{shape} {mode} norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for k in sref.MEANS:
        ok &= _within(f"{shape} {mode} {k}", abs(means[k] - float(m64[k])) / abs(float(m64[k])), abs(float(m32[k]) - float(m64[k])) / abs(float(m64[k])))
    assert ok


@pytest.mark.parametrize("shape,mode", [(s, m) for s in sref.SHAPES for m in ("mirror", "augment")])
def test_forward_outputs_are_the_policys_bit_for_bit(shape, mode):
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    sd, act, n, func, rows, idx = _case(shape, "scalar")
    crows = _cuda(rows)
    policy, ppo = _build(sd, act, "scalar", _sym(mode, func), learning_rate=1e-3, **ref.HYPER)
    obs, _ = func(obs=rows["observations"][idx], actions=None, env=None, obs_type="policy")
    cobs, _ = func(obs=rows["critic_observations"][idx], actions=None, env=None, obs_type="critic")
    want_mu, want_val = policy.act_inference(obs.to(DEV)).cpu(), policy.evaluate(cobs.to(DEV)).cpu()          # before the step changes the weights
    ppo.minibatch(crows, idx)
    mu, val = ppo.forward_outputs(n)
    K = ppo.num_blocks
    assert mu.shape == (K * n, policy.num_actions) and val.shape == ((K if mode == "augment" else 1) * n, 1)          # mirror only: the critic sees B rows
    assert torch.equal(mu, want_mu) and torch.equal(val, want_val[:val.shape[0]])
    plain_policy = NativeActorCritic(sd, act, noise_std_type="scalar", device=DEV, seed=1)
    plain = NativePPO(plain_policy, sd, learning_rate=1e-3, **ref.HYPER)
    plain.minibatch(crows, idx)
    pmu, pval = plain.forward_outputs(n)
    assert torch.equal(mu[:n], pmu) and torch.equal(val[:n], pval)


def _ulp(t):
    t = t.double().abs()
    return torch.where(t > 0, 2.0 ** (torch.floor(torch.log2(t.clamp_min(1e-300))) - 23), torch.full_like(t, 2.0 ** -149))


@pytest.mark.parametrize("mode", ["mirror", "both"])
def test_optimiser_step_on_the_kernels_own_gradients(mode):
    """The optimiser-step tolerance of tests/test_hip_ppo_update.py: 1e-5 lr + 1 ulp per parameter."""
    sd, act, n, func, rows, idx = _case("Y1", "scalar")
    hyper = dict(ref.HYPER, max_grad_norm=0.05, entropy_coef=0.01)
    lr = 2.5e-3
    policy, ppo = _build(sd, act, "scalar", _sym(mode, func), learning_rate=lr, **hyper)
    ppo.minibatch(_cuda(rows), idx)
    grads, norm, _ = ppo.gradients()
    assert norm > 0.05          # the clip bites
    want, _ = ref.clip_and_adam(sd, grads, ref.fresh_state(sd), lr, 0.05)
    after = ppo.optimizer_state()
    assert after["step"] == 1
    worst = 0.0
    for k in sd:
        tol = 1e-5 * lr + _ulp(want[k])
        worst = max(worst, float(((after["parameters"][k].double() - want[k]).abs() / tol).max()))
    print("largest |theta - theta64| / (1e-5 lr + 1 ulp):", worst)
    assert worst <= 1.0


def _elspider():
    from extended_legged_gym_amd.envs.elspider_air.elspider import get_symmetric_observation_action
    return get_symmetric_observation_action


@pytest.mark.parametrize("name", ["mirror", "augment", "both"])
def test_the_references_own_update(name):
    """tests/golden/ppo_symmetry_update.npz (the reference's `PPO.update` with its own ElSpider function on torch-CPU) through
    `NativeSymmetricPPO.update` with this repository's port of the function and the recorded permutation.  The learning rate must match exactly at
    every optimiser step (`both`: adaptive, it moves both ways, and the KL over all K B rows would leave the trajectory); the four loss means and the
    post-update action means and values are held to max(8 x the fp32-vs-fp64 deviation of the restatement, 2e-5), against float64 and against the
    reference's recorded values; collect -> update -> act uses the new weights without rebuilding."""
    from extended_legged_gym_amd.rl import NativeActorCritic
    case = sref.load_golden_case(name)
    sd, act, rows, perm, kw = case["sd0"], case["activation"], case["rows"], case["perm"], case["ppo"]
    hyper = {k: kw[k] for k in ref.HYPER}
    sym = dict(case["symmetry"], data_augmentation_func=_elspider(), _env=None)
    policy, ppo = _build(sd, act, case["noise_std_type"], sym, **kw)
    before = policy.act_inference(rows["observations"].to(DEV)).clone()
    loss = ppo.update(_cuda(rows), perm)
    print(name, "native", loss, ppo.learning_rate, "reference", case["loss"], case["learning_rate"])
    assert set(loss) == {"value_function", "surrogate", "entropy", "symmetry"}
    assert ppo.learning_rate == case["learning_rate"]
    _, loop = _build(sd, act, case["noise_std_type"], sym, **kw)
    mini, lrs = rows["observations"].shape[0] // kw["num_mini_batches"], []
    for _ in range(kw["num_learning_epochs"]):
        for i in range(kw["num_mini_batches"]):
            loop.minibatch(_cuda(rows), perm[i * mini:(i + 1) * mini])
            lrs.append(loop.optimizer_state()["learning_rate"])
    print(name, "learning-rate trajectory", lrs)
    assert lrs == case["lr_trajectory"]
    args = (sd, act, rows, perm, hyper, sym, kw["num_learning_epochs"], kw["num_mini_batches"], kw["learning_rate"])
    p64, l64, lr64, _, _ = sref.update(*args, torch.float64)
    p32, l32, lr32, _, _ = sref.update(*args, torch.float32)
    assert lr64 == case["learning_rate"]
    ok = True
    for k in ("value_function", "surrogate", "entropy", "symmetry"):
        ok &= _within(f"{name} loss {k} vs float64", abs(loss[k] - l64[k]) / abs(l64[k]), abs(l32[k] - l64[k]) / abs(l64[k]))
        ok &= _within(f"{name} loss {k} vs the reference", abs(loss[k] - case["loss"][k]) / abs(case["loss"][k]), abs(l32[k] - l64[k]) / abs(l64[k]))
    obs, cobs = rows["observations"], rows["critic_observations"]
    mu64, v64 = ref.mlp(p64, "actor", obs.double(), act), ref.mlp(p64, "critic", cobs.double(), act)
    mu32, v32 = ref.mlp(p32, "actor", obs, act), ref.mlp(p32, "critic", cobs, act)
    after = policy.act_inference(obs.to(DEV))
    ok &= _within(f"{name} action means", _err(after, mu64), _err(mu32, mu64))
    ok &= _within(f"{name} values", _err(policy.evaluate(cobs.to(DEV)), v64), _err(v32, v64))
    assert ok
    fresh = NativeActorCritic(ppo.state_dict(), act, noise_std_type=case["noise_std_type"], device=DEV, seed=1)
    assert torch.equal(after, fresh.act_inference(obs.to(DEV))) and not torch.equal(after, before)


def test_an_update_repeated_from_the_same_state_gives_equal_bits():
    case = sref.load_golden_case("both")
    sym = dict(case["symmetry"], data_augmentation_func=_elspider(), _env=None)
    rows = _cuda(case["rows"])
    _, one = _build(case["sd0"], case["activation"], case["noise_std_type"], sym, **case["ppo"])
    _, two = _build(case["sd0"], case["activation"], case["noise_std_type"], sym, **case["ppo"])
    loss1, loss2 = one.update(rows, case["perm"]), two.update(rows, case["perm"])
    assert loss1 == loss2 and one.kl == two.kl and one.learning_rate == two.learning_rate
    a, b = one.optimizer_state(), two.optimizer_state()
    assert a["step"] == b["step"] == case["ppo"]["num_learning_epochs"] * case["ppo"]["num_mini_batches"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


def test_refusals_from_python_and_at_the_c_abi():
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import NativePPO, NativeSymmetricPPO
    sd, act, n, func, rows, idx = _case("Y4", "scalar")
    sym = _sym("both", func)
    policy, ppo = _build(sd, act, "scalar", sym, max_rows=n - 1, **ref.HYPER)
    # a count above max_rows, at the C ABI
    r, _, keep = ppo._rows(_cuda(rows))
    didx, hyper = idx.to(DEV), ppo._hyper()
    rc = ppo.lib.lg_ppo_sym_minibatch(ppo.handle, C.byref(r), C.c_void_p(didx.data_ptr()), n, C.byref(hyper), None)
    msg = (ppo.lib.lg_mlp_last_error(None) or b"").decode()
    assert rc == abi.LG_ERR_INVALID and msg.startswith("lg_ppo_sym_minibatch: ") and "max_rows" in msg, (rc, msg)
    ppo.minibatch(_cuda(rows), idx[:n - 1])                      # the handle is still usable
    # tables the library must refuse, handed past the probe
    good = [tuple(a.copy() for a in t) for t in ppo._tables]

    def bad(which, edit):
        tabs = [tuple(a.copy() for a in t) for t in good]
        tabs[which] = edit(*tabs[which])
        return tabs

    def wider(p, s):
        return np.concatenate([p, p[:, :1]], axis=1), np.concatenate([s, s[:, :1]], axis=1)

    def out_of_range(p, s):
        p[1, 0] = p.shape[1]
        return p, s

    def half_sign(p, s):
        s[2, 1] = 0.5
        return p, s
    five = [(np.concatenate([p, p[1:3]]), np.concatenate([s, s[1:3]])) for p, s in good]
    for tabs, reason in ((five, "num_blocks 5"), (bad(0, wider), "observation table is 14 wide, the network takes 13"),
                         (bad(1, out_of_range), "critic observation table has an index out of range"), (bad(2, half_sign), r"action table has a sign that is not \+1 or -1")):
        with pytest.raises(RuntimeError, match="lg_ppo_sym_create: .*" + reason):
            ppo._create(n, tables=tabs)
    ppo._create(n)
    ppo.minibatch(_cuda(rows), idx)
    # from Python
    with pytest.raises(ValueError, match="at most 4"):
        NativeSymmetricPPO(policy, sd, symmetry_cfg=_sym("both", sref.synthetic_function((13, 9, 7), 5, 1)))
    with pytest.raises(NotImplementedError, match="symmetry_cfg"):
        NativePPO(policy, sd, symmetry_cfg=sym)
    for opt in ("normalize_advantage_per_mini_batch", "rnd_cfg", "multi_gpu_cfg"):
        with pytest.raises(NotImplementedError, match=opt):
            NativeSymmetricPPO(policy, sd, symmetry_cfg=sym, **{opt: True if opt.startswith("normalize") else {"x": 1}})

    class Recurrent:
        is_recurrent = True
    with pytest.raises(NotImplementedError, match="recurrent"):
        NativeSymmetricPPO(Recurrent(), sd, symmetry_cfg=sym)

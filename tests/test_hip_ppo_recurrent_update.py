"""The native recurrent PPO update (include/lgtrain_recurrent.h, `rl.NativeRecurrentPPO`) on the GPU against tests/ppo_recurrent_reference.py in
float64.  The bar of every gradient, norm and loss mean is the measured rule of tests/test_hip_ppo_update.py: e <= max(8 e32, 2e-5), e32 the
deviation of the restatement in fp32 from itself in float64 on the same inputs; both are printed before they are asserted.

Shapes, the smallest at which each part can go wrong:
  R1  LSTM, 1 layer, hidden 40 (a ragged 16-unit chunk), obs 20 / critic obs 24, T = 5, 37 envs (a ragged 32-row tile), log_std
  R2  GRU, 2 layers, hidden 40, the same rows: layer-to-layer dx and the split n gate
  R3  LSTM, 2 layers, hidden 64, T = 7, 75 envs: 525 rows = two full weight-gradient slabs and a ragged third
  R4  LSTM, 1 layer, hidden 512, obs 235, MLP [512, 256, 128], T = 3, 33 envs: the widest row, the LDS limit, two passes over D (4 x 512 columns)
  R5  T = 1 (101 envs); and R5b a mini-batch that is not the first slice (env0 = 37 of N = 2 x 37 + 5, GRU, 1 layer)
The backward tile (`rows_times_tiled`) walks the K = G H columns of the gate derivative D in passes of 1024; later passes add into dh_prev / dx, and a
GRU's z dh term and the zeroing of rows that entered from a saved state run in the last pass alone:
  R6  GRU, 1 layer, hidden 344: K = 1032, a GRU's two-pass backward, second pass of 8 columns
  R7  GRU, 2 layers, hidden 512: K = 1536, the whole n gate in pass two; dx of layer 1 across the edge
  R8  LSTM, 1 layer, hidden 257: K = 1028, second pass of 4 columns, not a whole 16-block
  R9  LSTM, 2 layers, hidden 260: K = 1040, second pass of one block, two layers
  R10 GRU, 1 layer, hidden 342, T = 4, 37 envs: K = 1026, second pass of 2 columns
  R11 LSTM, 1 layer, hidden 136, critic obs 33: 9 chunks, one ragged pass
  R12 GRU, 3 layers, hidden 9, obs 5 / critic obs 1, MLP [16]: H < 16, depth 3, a critic row of one column
tests/test_rnn_sweep_power.py shows on R6 - R10, without a GPU, that this bar sees a pass that is dropped, a pass that overwrites, and a lost z dh.
dones: `ppo_recurrent_reference.dones_pattern`, the issue's pattern scaled to the shape."""
import numpy as np
import pytest
import torch

from tests import ppo_recurrent_reference as rec
from tests import ppo_reference as ref
from tests.test_hip_ppo_update import _err, _ulp, _within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT = "elu"
SHAPES = {          # rnn_type, layers, hidden, obs, critic obs, MLP, T, N, env0, count, std key
    "R1": ("lstm", 1, 40, 20, 24, [32, 16], 5, 37, 0, 37, "log_std"),
    "R2": ("gru", 2, 40, 20, 24, [32, 16], 5, 37, 0, 37, "std"),
    "R3": ("lstm", 2, 64, 20, 24, [32, 16], 7, 75, 0, 75, "std"),
    "R4": ("lstm", 1, 512, 235, 235, [512, 256, 128], 3, 33, 0, 33, "std"),
    "R5": ("lstm", 1, 40, 20, 24, [32, 16], 1, 101, 0, 101, "std"),
    "R5b": ("gru", 1, 40, 20, 24, [32, 16], 5, 79, 37, 37, "log_std"),
    "R6": ("gru", 1, 344, 20, 24, [32, 16], 3, 33, 0, 33, "std"),
    "R7": ("gru", 2, 512, 48, 48, [64, 32], 3, 33, 0, 33, "std"),
    "R8": ("lstm", 1, 257, 20, 24, [32, 16], 3, 33, 0, 33, "std"),
    "R9": ("lstm", 2, 260, 17, 16, [32, 16], 3, 33, 0, 33, "std"),
    "R10": ("gru", 1, 342, 20, 24, [32, 16], 4, 37, 0, 37, "std"),
    "R11": ("lstm", 1, 136, 16, 33, [32, 16], 4, 37, 0, 37, "std"),
    "R12": ("gru", 3, 9, 5, 1, [16], 4, 37, 0, 37, "std"),
}
PASS_EDGE_SHAPES = ("R6", "R7", "R8", "R9", "R10")          # K > 1024: tests/test_rnn_sweep_power.py plants the backward's faults on these
SWEEP_SHAPES = PASS_EDGE_SHAPES + ("R11", "R12")          # the memory sweep's cases: their figures go to rnn_sweep.json (tests/test_hip_rnn_sweep.py)
_CACHE = {}


def _case(shape):
    """(state dict, rollout on the CPU, rnn_type, T, N, env0, count, std type): built once per shape and left unchanged."""
    if shape not in _CACHE:
        rnn_type, L, H, O, Oc, mlp, T, N, env0, count, std_key = SHAPES[shape]
        sd = rec.random_params(rnn_type, L, H, O, Oc, mlp, mlp, 12, seed=21, std_key=std_key)
        _CACHE[shape] = (sd, rec.craft_rollout(sd, ACT, rnn_type, T, N, seed=22), rnn_type, T, N, env0, count, "scalar" if std_key == "std" else "log")
    return _CACHE[shape]


def _native(ro):
    """A restatement rollout as the dict `collect_rollout` returns, on the device."""
    out = {k: ro[k].to(DEV) for k in rec.ROW_KEYS}
    out["dones"] = ro["dones"].to(DEV).unsqueeze(-1)
    for tag in ("a", "c"):
        h, c = ro["h_" + tag].to(DEV), ro["c_" + tag]
        out["hidden_states_" + tag] = (h, c.to(DEV)) if c is not None else h
    return out


def _build(sd, rnn_type, std_type, **kw):
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
    policy = NativeActorCriticRecurrent(sd, ACT, rnn_type, noise_std_type=std_type, device=DEV, seed=1)
    return policy, NativeRecurrentPPO(policy, sd, **kw)


GRAD_CASES = [("R1", True), ("R1", False), ("R2", True), ("R2", False), ("R3", True), ("R4", True), ("R4", False), ("R5", True), ("R5b", True), ("R5b", False),
              ("R6", True), ("R7", True), ("R7", False), ("R8", True), ("R9", True), ("R10", True), ("R10", False), ("R11", True), ("R12", True)]
FIGURES = {}          # shape -> the worst e / e32 and e / bar over its gradient tensors (tests/test_hip_rnn_sweep.py writes those of R6 - R12 out)


@pytest.mark.parametrize("shape,clipped", GRAD_CASES)
def test_gradients_losses_and_norm_against_float64(shape, clipped):
    sd, ro, rnn_type, T, N, env0, count, std_type = _case(shape)
    hyper = dict(ref.HYPER, use_clipped_value_loss=clipped, entropy_coef=0.01, value_loss_coef=0.8)
    policy, ppo = _build(sd, rnn_type, std_type, **hyper)
    ppo.minibatch(_native(ro), env0, count)
    g, norm, means = ppo.gradients()
    g64, n64, m64, ratio, dv, _, _ = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float64)
    g32, n32, m32, _, _, _, _ = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float32)
    adv = ro["advantages"][:, env0:env0 + count].reshape(-1).double()
    frac = ref.branch_fractions(ratio, dv, adv, hyper["clip_param"])
    print(shape, clipped, frac)
    assert min(frac[k] for k in ("pos_below", "pos_above", "neg_below", "neg_above")) >= 0.05 and min(frac["value_below"], frac["value_above"]) >= 0.10, frac
    assert set(g) == set(g64)
    ok = True
    for k in g64:
        e, e32 = _err(g[k], g64[k]), _err(g32[k], g64[k])
        ok &= _within(f"{shape} {k}", e, e32)
        fig = FIGURES.setdefault(shape, dict(e_over_e32=0.0, e_over_bar=0.0))
        fig.update(e_over_e32=max(fig["e_over_e32"], e / max(e32, 1e-300)), e_over_bar=max(fig["e_over_bar"], e / max(8.0 * e32, 2e-5)))
    ok &= _within(f"{shape} norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for k in ("surrogate", "value_function", "entropy", "kl"):
        ok &= _within(f"{shape} {k}", abs(means[k] - float(m64[k])) / abs(float(m64[k])), abs(float(m32[k]) - float(m64[k])) / abs(float(m64[k])))
    assert ok


def _forward(ppo, state, ro, env0, count):
    """The forward outputs of one mini-batch from the parameters of `state` (the step the call takes is undone first)."""
    ppo.load_optimizer_state(state)
    ppo.minibatch(_native(ro), env0, count)
    T = ro["observations"].shape[0]
    mu, val = ppo.forward_outputs(T * count)
    return mu.view(T, count, -1), val.view(T, count)


@pytest.mark.parametrize("shape", ["R1", "R2"])
def test_episode_boundaries_as_known_answers(shape):
    sd, ro, rnn_type, T, N, env0, count, std_type = _case(shape)
    policy, ppo = _build(sd, rnn_type, std_type, **ref.HYPER)
    ppo.minibatch(_native(ro), env0, count)
    state = dict(ppo.optimizer_state(), parameters=sd)
    mu0, v0 = _forward(ppo, state, ro, env0, count)
    d = ro["dones"]
    t, e = 1, 3          # dones_pattern(5, .): env 3 is done at steps 1 and 2, env 0 never
    assert d[t, e] == 1 and d[t + 1, e] == 1 and d[:, 0].sum() == 0
    # the restatement in fp32 and the kernels agree on the unchanged rollout to the forward tolerance
    mu64 = rec.forward(ref.cast(sd, torch.float64), ACT, rnn_type, rec.cast_rollout(ro, torch.float64), env0, count)[0]
    assert _err(mu0.reshape(T * count, -1), mu64) <= 2e-5
    other = dict(ro, observations=ro["observations"].clone(), critic_observations=ro["critic_observations"].clone())
    other["observations"][:t + 1, e] += 1.0
    other["critic_observations"][:t + 1, e] += 1.0
    mu1, v1 = _forward(ppo, state, other, env0, count)          # observations before a done: everything after it is bit-equal
    assert torch.equal(mu1[t + 1:], mu0[t + 1:]) and torch.equal(v1[t + 1:], v0[t + 1:])
    assert not torch.equal(mu1[:t + 1, e], mu0[:t + 1, e]) and not torch.equal(v1[:t + 1, e], v0[:t + 1, e])
    other = dict(ro, h_a=ro["h_a"].clone(), h_c=ro["h_c"].clone())
    other["h_a"][t + 1, :, e] += 0.5
    other["h_c"][t + 1, :, e] += 0.5
    mu2, v2 = _forward(ppo, state, other, env0, count)          # the saved row at a trajectory start is what the step enters with
    assert not torch.equal(mu2[t + 1, e], mu0[t + 1, e]) and not torch.equal(v2[t + 1, e], v0[t + 1, e])
    assert torch.equal(mu2[:t + 1], mu0[:t + 1])
    other = dict(ro, h_a=ro["h_a"].clone(), h_c=ro["h_c"].clone())
    other["h_a"][1:, :, 0] += 0.5
    other["h_c"][1:, :, 0] += 0.5
    mu3, v3 = _forward(ppo, state, other, env0, count)          # saved rows that are no start are never read
    assert torch.equal(mu3, mu0) and torch.equal(v3, v0)
    every = dict(ro, dones=torch.ones_like(d))          # every step of every env is a start and the saved rows are zero: h_in is zero everywhere
    for k in rec.STATE_KEYS:
        every[k] = torch.zeros_like(ro[k]) if ro[k] is not None else None
    ppo.load_optimizer_state(state)
    ppo.minibatch(_native(every), env0, count)
    g = ppo.gradients()[0]
    for k in g:
        if "weight_hh" in k:
            assert float(g[k].abs().max()) == 0.0, k
        if "weight_ih_l0" in k:
            assert float(g[k].abs().max()) > 0.0, k


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_trainer_and_acts_stay_coherent_on_a_collected_rollout(rnn_type):
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, collect_rollout
    from tests.test_env_api import make
    T, N, M = 8, 64, 2
    sd = rec.random_params(rnn_type, 2, 40, 48, 48, [64, 32], [64, 32], 12, seed=31)
    env = make("anymal_c_flat", N, **{"env.episode_length_s": 0.08, "seed": 5})          # 4 policy steps per episode: time-outs inside the rollout
    env.reset()
    policy, ppo = _build(sd, rnn_type, "scalar", learning_rate=3e-3, num_mini_batches=M, **ref.HYPER)
    policy.act_and_evaluate(env.obs_buf)          # one step lived: the first saved state is not zero
    out = collect_rollout(env, policy, T)
    assert float(out["dones"].sum()) > 0 and float(out["hidden_states_a"][0][0].abs().max() if rnn_type == "lstm" else out["hidden_states_a"][0].abs().max()) > 0
    mb = N // M
    ppo.minibatch(out, 0, mb)
    mu, val = ppo.forward_outputs(T * mb)          # unchanged parameters: the collected rows, bit for bit
    assert torch.equal(mu.view(T, mb, -1), out["mu"][:, :mb].cpu()) and torch.equal(val.view(T, mb, 1), out["values"][:, :mb].cpu())
    ppo.minibatch(out, mb, mb)
    new_sd = ppo.state_dict()
    assert set(new_sd) == set(sd)
    fresh = NativeActorCriticRecurrent(new_sd, ACT, rnn_type, device=DEV, seed=1)
    older = NativeActorCriticRecurrent(sd, ACT, rnn_type, device=DEV, seed=1)
    obs = out["observations"][0]
    for p in (policy, fresh, older):
        p.reset()
    a, b, c = policy.act_inference(obs), fresh.act_inference(obs), older.act_inference(obs)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(policy.evaluate(obs), fresh.evaluate(obs))
    assert torch.equal(policy.std.cpu(), new_sd["std"])
    for m, (prefix, mem) in enumerate((("memory_a", policy.memory_a), ("memory_c", policy.memory_c))):          # the device images against the host tiling
        for l in range(mem.num_layers):
            w, _ = ppo.images(m, l)
            wi, wh = (np.ascontiguousarray(new_sd[f"{prefix}.rnn.{n}_l{l}"].numpy()) for n in ("weight_ih", "weight_hh"))
            want = np.empty_like(w)
            assert ppo.lib.lg_rnn_tile_weights(abi.RNN_TYPES[rnn_type], wi.shape[1], 40, wi.ctypes.data, wh.ctypes.data, want.ctypes.data) == w.size
            assert np.array_equal(w, want), (prefix, l)


@pytest.mark.parametrize("max_grad_norm", [0.05, 1.0e3])
def test_optimiser_step_on_the_kernels_own_gradients(max_grad_norm):
    sd, ro, rnn_type, T, N, env0, count, std_type = _case("R2")
    hyper = dict(ref.HYPER, max_grad_norm=max_grad_norm, entropy_coef=0.01)
    lr = 2.5e-3
    policy, ppo = _build(sd, rnn_type, std_type, learning_rate=lr, **hyper)
    g = torch.Generator().manual_seed(8)
    state = dict(parameters=sd, exp_avg={k: 0.01 * torch.randn(v.shape, generator=g) for k, v in sd.items()},
                 exp_avg_sq={k: 1e-4 * torch.rand(v.shape, generator=g) for k, v in sd.items()}, step=7, learning_rate=lr)
    ppo.load_optimizer_state(state)
    back = ppo.optimizer_state()
    assert back["step"] == 7 and back["learning_rate"] == lr
    for k in sd:          # check / restore of the optimiser state round-trips
        assert torch.equal(back["exp_avg"][k], state["exp_avg"][k]) and torch.equal(back["parameters"][k], sd[k]) and torch.equal(back["exp_avg_sq"][k], state["exp_avg_sq"][k]), k
    ppo.minibatch(_native(ro), env0, count)
    grads, norm, _ = ppo.gradients()
    print("norm", norm, "max_grad_norm", max_grad_norm)
    assert (norm > max_grad_norm) == (max_grad_norm < 1.0)          # the clip bites in one case and not in the other
    want, wstate = ref.clip_and_adam(sd, grads, dict(exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"], step=7), lr, max_grad_norm)
    after = ppo.optimizer_state()
    assert after["step"] == 8
    worst = 0.0
    for k in sd:
        tol = 1e-5 * lr + _ulp(want[k])
        worst = max(worst, float(((after["parameters"][k].double() - want[k]).abs() / tol).max()))
        for moment in ("exp_avg", "exp_avg_sq"):
            assert float((after[moment][k].double() - wstate[moment][k]).abs().max()) <= 1e-6 * float(wstate[moment][k].abs().max()) + 1e-12, (moment, k)
    print("largest |theta - theta64| / (1e-5 lr + 1 ulp):", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["lstm", "gru"])
def test_the_references_own_update(name):
    """tests/golden/ppo_update_recurrent.npz (the reference's padded `PPO.update` on torch-CPU) through `NativeRecurrentPPO.update`: the learning rate
    exact after every optimiser step; losses, post-update action means and values within max(8 e32, 2e-5)."""
    case = rec.load_golden_case(name)
    sd, ro, kw = case["sd0"], case["rollout"], case["ppo"]
    hyper = {k: kw[k] for k in ref.HYPER}
    E, M = kw["num_learning_epochs"], kw["num_mini_batches"]
    policy, ppo = _build(sd, name, case["noise_std_type"], **kw)
    loss = ppo.update(_native(ro))
    print(name, "native", loss, ppo.learning_rate, "reference", case["loss"], case["learning_rate"])
    assert ppo.learning_rate == case["learning_rate"]
    _, loop = _build(sd, name, case["noise_std_type"], **kw)
    mb, lrs = ro["observations"].shape[1] // M, []
    for _ in range(E):
        for i in range(M):
            loop.minibatch(_native(ro), i * mb, mb)
            lrs.append(loop.optimizer_state()["learning_rate"])
    print(name, "learning-rate trajectory", lrs)
    assert lrs == case["lr_trajectory"]
    p64, l64, lr64, _, _ = rec.update(sd, ACT, name, ro, hyper, E, M, kw["learning_rate"], torch.float64)
    p32, l32, _, _, _ = rec.update(sd, ACT, name, ro, hyper, E, M, kw["learning_rate"], torch.float32)
    assert lr64 == case["learning_rate"]
    ok = True
    for k in ("value_function", "surrogate", "entropy"):
        ok &= _within(f"{name} loss {k} vs float64", abs(loss[k] - l64[k]) / abs(l64[k]), abs(l32[k] - l64[k]) / abs(l64[k]))
        ok &= _within(f"{name} loss {k} vs the reference", abs(loss[k] - case["loss"][k]) / abs(case["loss"][k]), abs(l32[k] - l64[k]) / abs(l64[k]))
    N = ro["observations"].shape[1]
    mu64, v64, _, _ = rec.forward(p64, ACT, name, rec.cast_rollout(ro, torch.float64), 0, N)
    mu32, v32, _, _ = rec.forward(p32, ACT, name, ro, 0, N)
    state = loop.optimizer_state()          # the post-update outputs of the SAME parameters: a forward-only look through one more (undone) mini-batch
    assert all(torch.equal(state["parameters"][k], v) for k, v in ppo.state_dict().items())
    loop.minibatch(_native(ro), 0, N)
    mu, val = loop.forward_outputs(ro["observations"].shape[0] * N)
    ok &= _within(f"{name} action means", _err(mu, mu64), _err(mu32, mu64))
    ok &= _within(f"{name} values", _err(val, v64), _err(v32, v64))
    assert ok


def _state_equal(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


def test_one_update_call_equals_the_loop_and_is_deterministic():
    sd, ro, rnn_type, T, N, _, _, std_type = _case("R5b")          # N = 79, M = 2: slices of 39 envs, one env unused
    E, M = 2, 2
    kw = dict(ref.HYPER, schedule="adaptive", desired_kl=0.004, entropy_coef=0.005, learning_rate=4e-3, num_learning_epochs=E, num_mini_batches=M)
    _, one = _build(sd, rnn_type, std_type, **kw)
    _, two = _build(sd, rnn_type, std_type, **kw)
    _, loop = _build(sd, rnn_type, std_type, **kw)
    rows = _native(ro)
    loss1, loss2 = one.update(rows), two.update(rows)
    mb, sums = N // M, dict(value_function=0.0, surrogate=0.0, entropy=0.0, kl=0.0)
    for _ in range(E):
        for i in range(M):
            loop.minibatch(rows, i * mb, mb)
            means = loop.gradients()[2]
            for k in sums:
                sums[k] += means[k]
    s1, s2, s3 = one.optimizer_state(), two.optimizer_state(), loop.optimizer_state()
    _state_equal(s1, s2)
    _state_equal(s1, s3)
    kl = sums.pop("kl") / (E * M)
    assert loss1 == loss2 and loss1 == {k: v / (E * M) for k, v in sums.items()}, (loss1, loss2, sums)
    assert one.kl == two.kl == kl
    assert one.learning_rate == two.learning_rate == s1["learning_rate"] == s3["learning_rate"] and s1["step"] == E * M
    changed = dict(rows, observations=rows["observations"].clone())
    changed["observations"][:, M * mb:] += 1.0          # the envs beyond M (N // M) are unused, as in the reference
    _, three = _build(sd, rnn_type, std_type, **kw)
    three.update(changed)
    _state_equal(s1, three.optimizer_state())


def test_refusals():
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeActorCriticRecurrent, NativeMemory, NativePPO, NativeRecurrentPPO
    sd, ro, rnn_type, T, N, env0, count, std_type = _case("R1")
    policy, ppo = _build(sd, rnn_type, std_type, **ref.HYPER)
    for opt in ("normalize_advantage_per_mini_batch", "rnd_cfg", "symmetry_cfg", "multi_gpu_cfg"):
        with pytest.raises(NotImplementedError, match=opt):
            NativeRecurrentPPO(policy, sd, **{opt: True if opt.startswith("normalize") else {"x": 1}})
    with pytest.raises(NotImplementedError, match="recurrent"):          # the feed-forward trainer keeps refusing a recurrent policy
        NativePPO(policy, sd)
    with pytest.raises(TypeError):
        NativeRecurrentPPO(NativeActorCritic({k: v for k, v in sd.items() if not k.startswith("memory")}, ACT, noise_std_type=std_type, device=DEV), sd)
    rows = _native(ro)
    for key in ("dones", "hidden_states_a", "hidden_states_c"):
        with pytest.raises(KeyError, match=key):
            ppo.update({k: v for k, v in rows.items() if k != key})
    # mismatched memory / MLP widths, refused by the library with the entry point's name
    wide = rec.random_params(rnn_type, 1, 48, 20, 24, [32, 16], [32, 16], 12, seed=23, std_key="log_std")
    odd = NativeActorCriticRecurrent(sd, ACT, rnn_type, noise_std_type=std_type, device=DEV)
    odd.memory_a = NativeMemory.from_state(wide, "memory_a", rnn_type, DEV)          # hidden 48 in front of an actor that reads 40
    with pytest.raises(RuntimeError, match="lg_ppo_recurrent_create: .*input width is not its memory's hidden width"):
        NativeRecurrentPPO(odd, dict(sd, **{k: v for k, v in wide.items() if k.startswith("memory_a")}), max_rows=64)
    other = "gru" if rnn_type == "lstm" else "lstm"
    gsd = rec.random_params(other, 1, 40, 20, 24, [32, 16], [32, 16], 12, seed=24, std_key="log_std")
    gpolicy = NativeActorCriticRecurrent(gsd, ACT, other, noise_std_type=std_type, device=DEV)
    with pytest.raises(ValueError, match="shapes"):          # LSTM parameters for GRU handles
        NativeRecurrentPPO(gpolicy, sd)
    claims = NativeRecurrentPPO(gpolicy, gsd)          # no handle yet
    gpolicy.memory_a.rnn_type = rnn_type          # the parameters now claim the other type than the handles have: refused by the library
    with pytest.raises(RuntimeError, match="lg_ppo_recurrent_create: .*rnn_type is not the memory handles'"):
        claims._create(64)
    gpolicy.memory_a.rnn_type = other
    claims.minibatch(_native(rec.craft_rollout(gsd, ACT, other, 2, 5, seed=25)), 0, 5)          # the refused handles still train
    ppo.minibatch(rows, env0, count)          # the refused calls left the first trainer usable

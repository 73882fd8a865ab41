"""GPU: the recurrent policy path (include/lgpolicy.h `lg_rnn_*`, `lg_policy_act_recurrent`, `lg_collect_rollout_recurrent`;
`NativeActorCriticRecurrent`) against the golden vectors of the reference's rsl_rl `ActorCriticRecurrent` and, at full size, against
`torch.nn.LSTM` / `nn.GRU` in float64 on the CPU.

Tolerance: the yardstick is the reference's OWN fp32-vs-float64 gap at step t (recorded in the golden file by the generator; computed here from
torch fp32 vs float64 for the full-size cases); the bar at step t is max(2e-5, 4 * yardstick[t]) absolute on outputs and hidden states, all O(1).
2e-5 is the feed-forward bar of tests/test_hip_policy.py (the MFMA k-chain); factor 4 = k-order differs from BLAS + the [x ; h] chain is twice as
long as either product + device exp / tanh differ from libm by a few ulp + one unit of head-room.  Step 0 from a zero state must hold 2e-5."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_recurrent.npz"))
FLOOR = 2e-5


def golden_state(name):
    base = name.split("_")[0]
    pre = base + ".sd."
    sd = {k[len(pre):]: torch.from_numpy(G[k].astype(np.float32)) for k in G.files if k.startswith(pre)}
    if name.endswith("_x3"):                         # the generator scaled the memory weights by 3 after rounding them to float16
        sd = {k: (3.0 * v if k.startswith("memory_") else v) for k, v in sd.items()}
    return sd, base


def bars(yardstick):
    return np.maximum(FLOOR, 4.0 * np.asarray(yardstick))


def check(tag, got, want, bar):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print(f"{tag}: max |err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (tag, err, bar)
    return err


@pytest.mark.parametrize("name", ["lstm", "gru", "lstm_x3", "gru_x3"])
def test_recurrent_actor_critic_matches_rsl_rl_golden(name):
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    sd, base = golden_state(name)
    ac = NativeActorCriticRecurrent(sd, activation="elu", rnn_type=base, device="cuda:0", seed=3)
    twin = NativeActorCriticRecurrent(sd, activation="elu", rnn_type=base, device="cuda:0", seed=3)       # driven through act, for action_mean
    assert ac.is_recurrent and ac.get_hidden_states() == (None, None)
    obs, cobs, dones = (torch.from_numpy(G[f"{base}.{k}"]).cuda() for k in ("obs", "cobs", "dones"))
    bar = bars(G[name + ".fp32_vs_fp64_maxabs"])
    assert bar[0] == FLOOR
    resets, twice = set(G["meta.reset_steps"].tolist()), int(G["meta.double_eval_step"])
    tags = ("h", "c") if base == "lstm" else ("h",)
    worst = np.zeros(len(bar))
    for t in range(len(bar)):
        e = [check(f"{name}[{t}] act_inference", ac.act_inference(obs[t]).cpu().numpy(), G[name + ".inference"][t], bar[t]),
             check(f"{name}[{t}] evaluate", ac.evaluate(cobs[t]).cpu().numpy(), G[name + ".value"][t], bar[t])]
        if t == twice:
            e.append(check(f"{name}[{t}] evaluate again", ac.evaluate(cobs[t]).cpu().numpy(), G[name + ".value_again"], bar[t]))
        _, values, _, mean, _ = twin.act_and_evaluate(obs[t], cobs[t])
        if t == twice:
            twin.evaluate(cobs[t])
        e.append(check(f"{name}[{t}] action_mean", mean.cpu().numpy(), G[name + ".mean"][t], bar[t]))
        assert mean is twin.action_mean
        ha, hc = ac.get_hidden_states()
        for mem, hs in (("a", ha), ("c", hc)):
            hs = hs if isinstance(hs, tuple) else (hs,)
            assert len(hs) == len(tags) and hs[0].shape == (2, 7, 40)
            for tag, h in zip(tags, hs):
                e.append(check(f"{name}[{t}] {tag}_{mem}", h.cpu().numpy(), G[f"{name}.{tag}_{mem}"][t], bar[t]))
        worst[t] = max(e)
        if t in resets:
            ac.reset(dones[t]); twin.reset(dones[t])
    print(f"{name}: per-step max |err| vs the golden: " + " ".join(f"{w:.2e}" for w in worst))
    with pytest.raises(NotImplementedError, match="PPO.update"):
        ac.act(obs[0], masks=torch.ones(1), hidden_states=None)
    with pytest.raises(NotImplementedError, match="PPO.update"):
        ac.evaluate(cobs[0], hidden_states=ac.get_hidden_states()[1])


class TorchRecurrent(torch.nn.Module):
    """The module tree of rsl_rl's ActorCriticRecurrent (state-dict names memory_a.rnn.*, memory_c.rnn.*, actor.*, critic.*, std) in plain torch."""

    def __init__(self, num_obs, num_actions, hidden, layers, mlp, rnn_type):
        super().__init__()
        cls = torch.nn.LSTM if rnn_type == "lstm" else torch.nn.GRU

        def seq(out):
            dims, mods = [hidden] + list(mlp), []
            for a, b in zip(dims[:-1], dims[1:]):
                mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
            return torch.nn.Sequential(*mods, torch.nn.Linear(dims[-1], out))
        self.memory_a, self.memory_c = torch.nn.Module(), torch.nn.Module()
        self.memory_a.rnn, self.memory_c.rnn = cls(num_obs, hidden, layers), cls(num_obs, hidden, layers)
        self.actor, self.critic = seq(num_actions), seq(1)
        self.std = torch.nn.Parameter(0.7 * torch.ones(num_actions))
        self.ha = self.hc = None

    def zero_rows(self, dones):
        for hs in (self.ha, self.hc):
            for h in (hs if isinstance(hs, tuple) else (hs,)):
                h[:, dones == 1, :] = 0.0

    def step(self, obs):
        with torch.no_grad():
            oa, self.ha = self.memory_a.rnn(obs.unsqueeze(0), self.ha)
            oc, self.hc = self.memory_c.rnn(obs.unsqueeze(0), self.hc)
            return self.actor(oa.squeeze(0)), self.critic(oc.squeeze(0))


@pytest.mark.parametrize("rnn_type,num_obs,hidden,layers,mlp,n", [("lstm", 235, 512, 1, [512, 256, 128], 4096 + 13), ("gru", 235, 512, 1, [512, 256, 128], 4096 + 13),
                                                                  ("lstm", 235, 512, 2, [512, 256, 128], 4096 + 13), ("gru", 235, 512, 2, [512, 256, 128], 4096 + 13),
                                                                  ("lstm", 48, 100, 2, [70, 33], 77), ("gru", 48, 100, 2, [70, 33], 77)])
def test_full_size_against_float64(rnn_type, num_obs, hidden, layers, mlp, n):
    """8 steps with ~5 % random dones against torch in float64 on the CPU with the same weights; the yardstick is torch fp32 vs float64 on the same inputs."""
    import copy
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    torch.manual_seed(7)
    ref32 = TorchRecurrent(num_obs, 12, hidden, layers, mlp, rnn_type)
    ref64 = copy.deepcopy(ref32).double()
    ac = NativeActorCriticRecurrent(ref32.state_dict(), "elu", rnn_type, device="cuda:0", seed=5)
    g = torch.Generator().manual_seed(2)
    worst, yard = [], []
    for t in range(8):
        obs = torch.randn(n, num_obs, generator=g)
        dones = (torch.rand(n, generator=g) < 0.05).float()
        m32, v32 = ref32.step(obs)
        m64, v64 = ref64.step(obs.double())
        _, values, _, mean, _ = ac.act_and_evaluate(obs.cuda())
        ha, hc = ac.get_hidden_states()
        got = [mean, values] + list(ha if isinstance(ha, tuple) else (ha,)) + list(hc if isinstance(hc, tuple) else (hc,))
        w32 = [m32, v32] + list(ref32.ha if isinstance(ref32.ha, tuple) else (ref32.ha,)) + list(ref32.hc if isinstance(ref32.hc, tuple) else (ref32.hc,))
        w64 = [m64, v64] + list(ref64.ha if isinstance(ref64.ha, tuple) else (ref64.ha,)) + list(ref64.hc if isinstance(ref64.hc, tuple) else (ref64.hc,))
        y = max(float((a.double() - b).abs().max()) for a, b in zip(w32, w64))
        bar = max(FLOOR, 4.0 * y) if t > 0 else FLOOR
        e = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(got, w64))
        print(f"{rnn_type} x{layers} hidden {hidden} step {t}: max |err| vs float64 {e:.3e}; torch fp32 vs float64 {y:.3e}; bar {bar:.3e}")
        worst.append(e); yard.append(y)
        assert e <= bar, (t, e, bar)
        ref32.zero_rows(dones); ref64.zero_rows(dones); ac.reset(dones.cuda())
    print(f"{rnn_type} x{layers} hidden {hidden}: per-step max |err| " + " ".join(f"{w:.2e}" for w in worst) + " | yardstick " + " ".join(f"{w:.2e}" for w in yard))


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_reset_is_exact(rnn_type):
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    torch.manual_seed(1)
    sd = TorchRecurrent(48, 12, 100, 2, [64, 32], rnn_type).state_dict()
    n = 70
    g = torch.Generator().manual_seed(3)
    obs = [torch.randn(n, 48, generator=g).cuda() for _ in range(4)]
    dones = (torch.rand(n, generator=g) < 0.3).float().cuda()
    assert 0 < int(dones.sum()) < n
    done = dones.bool()
    a, b, fresh, folded = (NativeActorCriticRecurrent(sd, "elu", rnn_type, device="cuda:0", seed=2) for _ in range(4))
    for t in range(3):
        for p in (a, b, folded):
            p.act_inference(obs[t]); p.evaluate(obs[t])
    a.reset(dones)                                     # b: no reset call
    out_a, val_a = a.act_inference(obs[3]).clone(), a.evaluate(obs[3]).clone()
    out_b, val_b = b.act_inference(obs[3]).clone(), b.evaluate(obs[3]).clone()
    out_f, val_f = fresh.act_inference(obs[3]).clone(), fresh.evaluate(obs[3]).clone()
    assert torch.equal(out_a[done], out_f[done]) and torch.equal(val_a[done], val_f[done])          # a done row = a fresh policy on the same row
    assert torch.equal(out_a[~done], out_b[~done]) and torch.equal(val_a[~done], val_b[~done])      # the others never noticed
    assert not torch.equal(out_b[done], out_f[done])
    # the reset mask folded into the step (lg_rnn_step's `reset`) is the stand-alone reset followed by the step
    top = folded.memory_a(obs[3], reset=dones)
    assert torch.equal(folded.actor(top), out_a)
    for x, y in zip(folded.memory_a.hidden_states if rnn_type == "lstm" else (folded.memory_a.hidden_states,),
                    a.memory_a.hidden_states if rnn_type == "lstm" else (a.memory_a.hidden_states,)):
        assert torch.equal(x, y)
    # reset() forgets everything; a new row count re-allocates a zero state
    a.reset()
    assert a.get_hidden_states() == (None, None)
    assert torch.equal(a.act_inference(obs[3]), out_f)
    a.act_inference(obs[3][:5])
    assert a.memory_a.h.shape == (2, 5, 100)


def test_recurrent_policy_draws_the_feed_forward_noise():
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeActorCriticRecurrent
    torch.manual_seed(4)
    rec = TorchRecurrent(48, 12, 64, 1, [64, 32], "lstm")
    sd = rec.state_dict()
    ff = {k: v for k, v in sd.items() if not k.startswith("memory_")}
    n = 300
    obs = torch.randn(n, 48).cuda()
    r = NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=11)
    f = NativeActorCritic(ff, "elu", device="cuda:0", seed=11)
    for call in range(3):
        ar, _, lpr, mr, sr = r.act_and_evaluate(obs)
        af, _, _, mf, sf = f.act_and_evaluate(torch.randn(n, 64).cuda())
        zr, zf = (ar - mr) / sr, (af - mf) / sf
        assert torch.allclose(zr, zf, rtol=0, atol=2e-6)            # the same draw, up to the rounding of (mean + sigma z - mean) / sigma around two different means
        want = (-((ar - mr) ** 2) / (2 * sr * sr) - torch.log(sr) - 0.9189385332046727).sum(-1)
        np.testing.assert_allclose(lpr.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4)
    # with equal means the actions themselves are bit-equal: feed the feed-forward actor the memory's output
    r2 = NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=11)
    f2 = NativeActorCritic(ff, "elu", device="cuda:0", seed=11)
    a2 = r2.act(obs).clone()
    top = r2.memory_a.h[-1].clone()
    af2, _, _, mf2, sf2 = f2.act_and_evaluate(top, torch.zeros(n, 64).cuda())
    assert torch.equal(a2, af2) and torch.equal(r2.action_mean, mf2)
    assert torch.equal((a2 - r2.action_mean) / r2.action_std, (af2 - mf2) / sf2)
    assert torch.equal(r2.get_actions_log_prob(r2._actions), f2.get_actions_log_prob(af2))          # both: the launch's own log-prob of its own draw
    assert r2.memory_c.h is None                                     # act alone leaves the critic memory to evaluate


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_collect_rollout_recurrent_matches_the_python_loop(rnn_type):
    """`lg_collect_rollout_recurrent` against act_and_evaluate -> env.step -> reset(dones) driven from Python on two identically seeded envs, T = 24:
    every row, both hidden-state stacks and the final memory state bit for bit (the pattern of test_collect_rollout_matches_the_python_loop)."""
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, collect_rollout, compute_returns
    from tests.test_env_api import make
    T, N = 24, 256
    torch.manual_seed(3)
    sd = TorchRecurrent(48, 12, 40, 2, [64, 32], rnn_type).state_dict()
    over = {"env.episode_length_s": 0.08, "seed": 5}       # max_episode_length = 4 policy steps: time-outs inside the rollout
    envs = [make("anymal_c_flat", N, **over) for _ in range(2)]
    acs = [NativeActorCriticRecurrent(sd, "elu", rnn_type, device="cuda:0", seed=11) for _ in range(2)]
    for e in envs:
        e.reset()
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf)

    def flat(hs):
        return list(hs) if isinstance(hs, tuple) else [hs]
    # both policies have already lived one step, so the first saved state is not all zeros
    for ac in acs:
        ac.act_and_evaluate(envs[0].obs_buf)
    env, ac = envs[0], acs[0]
    rows = {k: [] for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob", "mu", "sigma")}
    hid_a, hid_c = [], []
    obs = env.get_observations()
    for t in range(T):
        ha, hc = ac.get_hidden_states()
        hid_a.append([h.clone() for h in flat(ha)]); hid_c.append([h.clone() for h in flat(hc)])
        a, v, lp, mu, sig = ac.act_and_evaluate(obs)
        rows["observations"].append(obs.clone()); rows["actions"].append(a.clone()); rows["values"].append(v.clone())
        rows["actions_log_prob"].append(lp.clone().view(-1, 1)); rows["mu"].append(mu.clone()); rows["sigma"].append(sig.clone())
        obs, _, rew, dones, infos = env.step(a)
        r = rew.clone()
        r += 0.99 * torch.squeeze(v * infos["time_outs"].unsqueeze(1), 1)            # ppo.py:179-183
        rows["rewards"].append(r.view(-1, 1)); rows["dones"].append(dones.float().view(-1, 1))
        ac.reset(dones)                                                              # ppo.py:188
    ref = {k: torch.stack(v) for k, v in rows.items()}
    last = ac.evaluate(obs)                                                          # ppo.py:190-192: advances the critic memory
    ret, adv = compute_returns(ref["rewards"], ref["dones"], ref["values"], last, 0.99, 0.95, True)
    out = collect_rollout(envs[1], acs[1], T, 0.99, 0.95, True)
    torch.cuda.synchronize()
    assert float(ref["dones"].sum()) > 0
    for k in ref:
        assert torch.equal(out[k], ref[k]), (k, float((out[k] - ref[k]).abs().max()))
    assert torch.equal(out["last_values"], last) and torch.equal(out["returns"], ret) and torch.equal(out["advantages"], adv)
    for key, want in (("hidden_states_a", hid_a), ("hidden_states_c", hid_c)):
        got = flat(out[key])
        assert len(got) == (2 if rnn_type == "lstm" else 1)
        for j, stack in enumerate(got):
            assert stack.shape == (T, 2, N, 40) and torch.equal(stack, torch.stack([w[j] for w in want])), key
        assert float(got[0][0].abs().max()) > 0 and float((got[0][5][:, ref["dones"][4, :, 0] == 1] != 0).sum()) == 0       # done rows enter the next step zeroed
    for x, y in zip(flat(acs[0].get_hidden_states()[0]) + flat(acs[0].get_hidden_states()[1]), flat(acs[1].get_hidden_states()[0]) + flat(acs[1].get_hidden_states()[1])):
        assert torch.equal(x, y)
    assert torch.equal(envs[0].obs_buf, envs[1].obs_buf) and acs[0]._call == acs[1]._call == T + 1
    assert envs[0].common_step_counter == envs[1].common_step_counter


def test_planner_warm_start_with_an_lstm_actor(tmp_path):
    """`rl_warmstart.actor_network = "lstm"`: the env constructs from an `ActorCriticRecurrent`-shaped checkpoint, the warm start's nodes are `u2node` applied to
    the actions a float64 torch copy of the actor produces on the observations the policy saw (from a zero memory), and a second warm start from the same
    observation rows gives the same nodes: the memory was reset.  (The rollout sync copies simulator state, not observation rows -- see
    tests/test_traj_sampler.py -- so the rows are put back before the second call.)"""
    import copy
    from extended_legged_gym_amd.envs.anymal_c.batch_rollout.anymal_c_batch_rollout_config import AnymalCBatchRolloutCfg
    from extended_legged_gym_amd.envs.batch_rollout.robot_traj_grad_sampling import RobotTrajGradSampling
    from extended_legged_gym_amd.envs.batch_rollout.robot_traj_grad_sampling_config import RobotTrajGradSamplingCfg
    from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args, parse_sim_params
    cfg = AnymalCBatchRolloutCfg()
    cfg.trajectory_opt = RobotTrajGradSamplingCfg.trajectory_opt()
    cfg.rl_warmstart = RobotTrajGradSamplingCfg.rl_warmstart()
    cfg.env.num_envs, cfg.env.rollout_envs = 6, 16
    cfg.noise.add_noise = False; cfg.domain_rand.push_robots = False; cfg.domain_rand.randomize_friction = False
    cfg.seed = 5
    num_obs = cfg.env.num_observations
    torch.manual_seed(0)
    ref32 = TorchRecurrent(num_obs, 12, 64, 1, [64, 32], "lstm")
    with torch.no_grad():
        for p in ref32.actor.parameters():
            p.mul_(0.3)
    path = str(tmp_path / "model_10.pt")
    torch.save({"model_state_dict": ref32.state_dict(), "iter": 10, "infos": None}, path)
    rl = cfg.rl_warmstart
    rl.enable, rl.policy_checkpoint, rl.obs_type, rl.actor_network = True, path, "non_privileged", "lstm"
    sim_params = parse_sim_params(get_args([]), {"sim": class_to_dict(cfg.sim)})
    env = RobotTrajGradSampling(cfg, sim_params, "native_hip", "cuda:0", True)
    env.reset()
    for _ in range(5):
        env.step(torch.zeros(6, 12, device=env.device))
    s = env.traj_grad_sampler
    assert s.rl_policy.is_recurrent and s.use_rl_warmstart and not s.mean.any()
    s.rl_policy.act_inference(env.obs_buf[env.main_env_indices + 1])          # leave some state behind: the warm start must not inherit it
    seen, inner = [], s._policy_action
    s._policy_action = lambda obs: (seen.append(obs.clone()), inner(obs))[1]
    rows_before = env.obs_buf.clone()
    env._init_trajectories_from_rl()
    nodes1, seen1 = s.mean.clone(), list(seen)
    assert s.rl_traj_initialized and nodes1.shape == (6, s.K, 12) and torch.isfinite(nodes1).all() and float(nodes1.abs().max()) > 1e-3
    assert len(seen1) == s.H + 1

    def torch_nodes(ref, dtype):
        ref.ha = ref.hc = None
        acts = torch.stack([ref.step(o.cpu().to(dtype))[0] for o in seen1], dim=1)          # (M, H + 1, A)
        return torch.einsum("kh,mha->mka", s.u2node.cpu().to(dtype), acts[:, :s.H])
    n64 = torch_nodes(copy.deepcopy(ref32).double(), torch.float64)
    yard = float((torch_nodes(ref32, torch.float32).double() - n64).abs().max())
    err = float((nodes1.cpu().double() - n64).abs().max())
    print(f"warm start nodes: max |err| vs float64 {err:.3e}; torch fp32 vs float64 {yard:.3e}")
    assert err <= max(FLOOR, 4.0 * yard)
    seen.clear()
    env.obs_buf.copy_(rows_before)
    env._init_trajectories_from_rl()
    assert all(torch.equal(x, y) for x, y in zip(seen, seen1)), "the second roll-out saw other observations: not a test of the memory"
    assert torch.equal(s.mean, nodes1)
    with pytest.raises(ValueError, match="actor_network"):
        rl.actor_network = "transformer"
        s.init_rl_policy(rl, num_obs)

"""A torch restatement of one mini-batch step and of the whole `PPO.update` of the vendored rsl_rl for `ActorCriticRecurrent`
(`algorithms/ppo.py:197-438` with the mini-batches of `storage/rollout_storage.py:246-316`), in the UNPADDED formulation the native update uses:
the env slice `[env0, env0 + count)` is walked in time order, the gates are written out, and row j enters step t with the saved hidden row
`hidden[t][:, env0 + j]` when `t == 0` or `dones[t - 1, env0 + j] != 0`, else with its own state after step t - 1.  Autograd gives the gradients;
the losses, `clip_grad_norm_`'s rule and the hand-written Adam are `tests/ppo_reference.py`'s.  dtype-generic, as that file.
`tests/test_ppo_recurrent_reference.py` holds this file to the reference's own padded `PPO.update` (tests/golden/ppo_update_recurrent.npz)."""
import json
import os

import numpy as np
import torch

from tests import ppo_reference as ref

ROW_KEYS = ref.ROW_KEYS
STATE_KEYS = ("h_a", "c_a", "h_c", "c_c")


def num_layers(params, prefix):
    return len([k for k in params if k.startswith(prefix + ".rnn.weight_ih_l")])


def cell(params, prefix, l, rnn_type, x, h, c):
    """One step of layer l of nn.LSTM / nn.GRU: (h', c')."""
    p = lambda name: params[f"{prefix}.rnn.{name}_l{l}"]          # noqa: E731
    gi = torch.nn.functional.linear(x, p("weight_ih"), p("bias_ih"))
    gh = torch.nn.functional.linear(h, p("weight_hh"), p("bias_hh"))
    H = h.shape[-1]
    if rnn_type == "lstm":
        g = gi + gh
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c2 = f * c + i * gg
        return o * torch.tanh(c2), c2
    r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h, None


def memory_forward(params, prefix, rnn_type, x, h_rows, c_rows, dones):
    """x (T, n, I); h_rows / c_rows (T, L, n, H): the saved state BEFORE each step (c_rows None for a GRU); dones (T, n).  Returns the top layer's h'
    (T, n, H) under the entering-state rule above."""
    T, L = x.shape[0], num_layers(params, prefix)
    h = [None] * L
    c = [None] * L
    out = []
    for t in range(T):
        start = torch.ones_like(dones[0], dtype=torch.bool) if t == 0 else dones[t - 1] != 0
        inp = x[t]
        for l in range(L):
            hin = h_rows[t, l] if t == 0 else torch.where(start[:, None], h_rows[t, l], h[l])
            cin = None
            if rnn_type == "lstm":
                cin = c_rows[t, l] if t == 0 else torch.where(start[:, None], c_rows[t, l], c[l])
            h[l], c[l] = cell(params, prefix, l, rnn_type, inp, hin, cin)
            inp = h[l]
        out.append(inp)
    return torch.stack(out)


def slice_batch(rollout, env0, count):
    """The mini-batch of env slice [env0, env0 + count): rows flattened time-major (the reference's (T, count) flatten), states and dones sliced."""
    rows = {k: rollout[k][:, env0:env0 + count].reshape(-1, rollout[k].shape[-1]) for k in ROW_KEYS if k in rollout}
    states = {k: (rollout[k][:, :, env0:env0 + count] if rollout.get(k) is not None else None) for k in STATE_KEYS}
    return rows, states, rollout["dones"][:, env0:env0 + count]


def forward(params, act, rnn_type, rollout, env0, count):
    """(action means (T * count, A), values (T * count, 1)) of the slice, time-major."""
    T = rollout["observations"].shape[0]
    obs, cobs = rollout["observations"][:, env0:env0 + count], rollout["critic_observations"][:, env0:env0 + count]
    _, states, dones = slice_batch(rollout, env0, count)
    top_a = memory_forward(params, "memory_a", rnn_type, obs, states["h_a"], states["c_a"], dones).reshape(T * count, -1)
    top_c = memory_forward(params, "memory_c", rnn_type, cobs, states["h_c"], states["c_c"], dones).reshape(T * count, -1)
    return ref.mlp(params, "actor", top_a, act), ref.mlp(params, "critic", top_c, act), top_a, top_c


def cast_rollout(rollout, dtype):
    return {k: (v.detach().to(dtype).clone() if v is not None else None) for k, v in rollout.items()}


def gradients(params, act, rnn_type, rollout, env0, count, hyper, dtype=torch.float64):
    """Pre-clip gradients of one mini-batch in `dtype`: (gradients, global norm, loss means, ratio, value difference, action means, values)."""
    p = {k: v.requires_grad_(True) for k, v in ref.cast(params, dtype).items()}
    ro = cast_rollout(rollout, dtype)
    mu, val, top_a, top_c = forward(p, act, rnn_type, ro, env0, count)
    rows, _, _ = slice_batch(ro, env0, count)
    batch = dict(rows, observations=top_a, critic_observations=top_c)
    loss, means, ratio, dv = ref.loss_terms(p, act, batch, hyper)
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    norm = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
    return grads, norm, means, ratio, dv, mu.detach(), val.detach()


def update(params, act, rnn_type, rollout, hyper, num_learning_epochs, num_mini_batches, learning_rate, dtype=torch.float64, state=None):
    """The whole recurrent `PPO.update`: (params, loss dict, final learning rate, trace, optimiser state); the slices are the same in every epoch."""
    params = ref.cast(params, dtype)
    state = state if state is not None else ref.fresh_state(params, dtype)
    N = rollout["observations"].shape[1]
    mb = N // num_mini_batches
    lr = learning_rate
    sums = dict(value_function=0.0, surrogate=0.0, entropy=0.0)
    trace = []
    for _ in range(num_learning_epochs):
        for i in range(num_mini_batches):
            grads, norm, means, ratio, dv, _, _ = gradients(params, act, rnn_type, rollout, i * mb, mb, hyper, dtype)
            if hyper["schedule"] == "adaptive":
                lr = ref.adaptive_learning_rate(lr, float(means["kl"]), hyper["desired_kl"])
            params, state = ref.clip_and_adam(params, grads, state, lr, hyper["max_grad_norm"], dtype)
            for k in sums:
                sums[k] += float(means[k])
            trace.append(dict(learning_rate=lr, kl=float(means["kl"]), ratio=ratio, dv=dv, norm=float(norm)))
    n = num_learning_epochs * num_mini_batches
    return params, {k: v / n for k, v in sums.items()}, lr, trace, state


def random_params(rnn_type, layers, hidden, obs, critic_obs, actor_dims, critic_dims, actions, seed, std_key="std", std=0.7):
    """An `ActorCriticRecurrent` state dict with torch's uniform initialisation scale (1 / sqrt(hidden)), seeded."""
    g = torch.Generator().manual_seed(seed)
    G = 4 if rnn_type == "lstm" else 3
    sd = {}
    for prefix, dims in (("actor", [hidden] + list(actor_dims) + [actions]), ("critic", [hidden] + list(critic_dims) + [1])):
        for j in range(len(dims) - 1):
            bound = 1.0 / np.sqrt(dims[j])
            sd[f"{prefix}.{2 * j}.weight"] = (torch.rand(dims[j + 1], dims[j], generator=g) * 2 - 1) * bound * 1.7
            sd[f"{prefix}.{2 * j}.bias"] = (torch.rand(dims[j + 1], generator=g) * 2 - 1) * bound
    s = std * (1.0 + 0.2 * torch.rand(actions, generator=g))
    sd[std_key] = s if std_key == "std" else torch.log(s)
    bound = 1.0 / np.sqrt(hidden)
    for prefix, width in (("memory_a", obs), ("memory_c", critic_obs)):
        for l in range(layers):
            I = width if l == 0 else hidden
            for name, shape in (("weight_ih", (G * hidden, I)), ("weight_hh", (G * hidden, hidden)), ("bias_ih", (G * hidden,)), ("bias_hh", (G * hidden,))):
                sd[f"{prefix}.rnn.{name}_l{l}"] = (torch.rand(*shape, generator=g) * 2 - 1) * bound * 1.5
    return sd


def dones_pattern(T, N):
    """The pattern of the issue's check, scaled to (T, N): a done at t = 0, at t = T - 1, at consecutive steps, one env done at every step, several
    envs never done.  Returns (T, N) float32."""
    d = torch.zeros(T, N)
    base = [(0, 1), (7, 2), (3, 3), (4, 3), (6, 4), (2, 5), (5, 5), (1, 9)]
    for rep in range(0, N, 12):
        for t, e in base:
            tt = t if T == 8 else (t * (T - 1)) // 7          # 0 and T - 1 stay the ends, steps 3 and 4 stay consecutive
            if rep + e < N:
                d[tt, rep + e] = 1.0
        if rep + 6 < N:
            d[:, rep + 6] = 1.0
    return d


def collect_states(params, rnn_type, obs, cobs, dones, seed):
    """The hidden rows a collection keeps: the memories are warmed by one step on seeded rows (the state at t = 0 is not zero), then per step the
    state is saved, the memory steps, and the rows with dones[t] are zeroed (`ppo.py:148-149, 188`).  (T, L, N, H) per tensor; c None for a GRU."""
    g = torch.Generator().manual_seed(seed)
    T, N = obs.shape[:2]
    out = {}
    for prefix, x, tag in (("memory_a", obs, "a"), ("memory_c", cobs, "c")):
        L = num_layers(params, prefix)
        H = params[f"{prefix}.rnn.weight_hh_l0"].shape[1]
        h = [torch.zeros(N, H) for _ in range(L)]
        c = [torch.zeros(N, H) for _ in range(L)]
        hs, cs = [], []
        for t in range(-1, T):
            inp = torch.randn(N, x.shape[-1], generator=g) if t < 0 else x[t]
            if t >= 0:
                hs.append(torch.stack(h)); cs.append(torch.stack(c))
            for l in range(L):
                h[l], c2 = cell(params, prefix, l, rnn_type, inp, h[l], c[l])
                c[l] = c2 if c2 is not None else c[l]
                inp = h[l]
            if t >= 0:
                keep = (dones[t] == 0).float()[:, None]
                h, c = [v * keep for v in h], [v * keep for v in c]
        out["h_" + tag] = torch.stack(hs)
        out["c_" + tag] = torch.stack(cs) if rnn_type == "lstm" else None
    return out


def craft_rollout(params, act, rnn_type, T, N, seed, dones=None, kl_scale=0.05, ratio_spread=0.35, value_spread=0.3):
    """A seeded float32 (T, N, .) rollout around the CURRENT policy, by the recipe of `ppo_reference.craft_rows`: the stored log-probs, values, means
    and sigmas sit where every branch of the clipped losses is populated at the first step.  Keys: ROW_KEYS, dones (T, N), STATE_KEYS."""
    g = torch.Generator().manual_seed(seed)
    p = ref.cast(params, torch.float32)
    O, Oc = p["memory_a.rnn.weight_ih_l0"].shape[1], p["memory_c.rnn.weight_ih_l0"].shape[1]
    dones = dones_pattern(T, N) if dones is None else dones
    obs, cobs = torch.randn(T, N, O, generator=g), torch.randn(T, N, Oc, generator=g)
    with torch.no_grad():
        ro = dict(observations=obs, critic_observations=cobs, dones=dones, **collect_states(p, rnn_type, obs, cobs, dones, seed + 1))
        mu_now, v_now, _, _ = forward(p, act, rnn_type, ro, 0, N)
        sigma_now = ref.sigma_of(p).expand_as(mu_now)
        mu = mu_now + kl_scale * sigma_now * torch.randn(mu_now.shape, generator=g)
        sigma = (sigma_now * (1.0 + 0.5 * kl_scale)).contiguous()
        actions = mu + sigma * torch.randn(mu_now.shape, generator=g)
        logp_now = (-((actions - mu_now) ** 2) / (2 * sigma_now ** 2) - torch.log(sigma_now) - ref.LOG_SQRT_2PI).sum(-1, keepdim=True)
        R = T * N
        logp = logp_now - ratio_spread * torch.randn(R, 1, generator=g)
        values = v_now + value_spread * torch.randn(R, 1, generator=g)
        returns = values + torch.randn(R, 1, generator=g)
        adv = torch.randn(R, 1, generator=g)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    flat = dict(actions=actions, values=values, returns=returns, advantages=adv, actions_log_prob=logp, mu=mu, sigma=sigma)
    ro.update({k: v.reshape(T, N, -1).contiguous() for k, v in flat.items()})
    return ro


def load_golden_case(name):
    """A case of tests/golden/ppo_update_recurrent.npz (tools/refgen/make_ppo_update_recurrent_golden.py): the state dict before (`sd0`) and after
    (`sd1`) the reference's `PPO.update`, the rollout (rows, dones, hidden rows), the loss dict, the learning rate after every step, the settings."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_update_recurrent.npz"))
    part = lambda tag: {k[len(name) + len(tag) + 2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(f"{name}.{tag}.")}  # noqa: E731
    cfg = json.loads(str(z[f"{name}.config"]))
    rollout = part("rollout")
    for k in STATE_KEYS:
        rollout.setdefault(k, None)
    loss = dict(zip(("value_function", "surrogate", "entropy"), [float(x) for x in z[f"{name}.loss"]]))
    return dict(sd0=part("sd0"), sd1=part("sd1"), rollout=rollout, loss=loss, learning_rate=float(z[f"{name}.learning_rate"]),
                lr_trajectory=[float(x) for x in z[f"{name}.lr_trajectory"]], **cfg)

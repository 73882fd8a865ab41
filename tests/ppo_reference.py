"""A torch restatement of one mini-batch step and of the whole `PPO.update` of the vendored rsl_rl (`algorithms/ppo.py:197-438`, mini-batches as
`storage/rollout_storage.py:184-243`) for the feed-forward `ActorCritic`: autograd for the gradients, `clip_grad_norm_`'s rule and a hand-written
Adam (torch's defaults).  dtype-generic: float64 is the reference the native update is held to, float32 is "torch's own fp32" whose deviation from
float64 sets the bar.  `tests/test_ppo_update_reference.py` holds this file to the reference's own `PPO.update` (tests/golden/ppo_update.npz)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ACTS = {"elu": F.elu, "relu": F.relu, "tanh": torch.tanh, "lrelu": F.leaky_relu, "selu": F.selu}
ROW_KEYS = ("observations", "critic_observations", "actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma")
HYPER = dict(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.0, use_clipped_value_loss=True, max_grad_norm=1.0, desired_kl=0.01, schedule="fixed")
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def layer_names(params, prefix):
    return sorted({int(k.split(".")[1]) for k in params if k.startswith(prefix + ".") and k.endswith(".weight")})


def mlp(params, prefix, x, act):
    idx = layer_names(params, prefix)
    for j, i in enumerate(idx):
        x = F.linear(x, params[f"{prefix}.{i}.weight"], params[f"{prefix}.{i}.bias"])
        if j < len(idx) - 1:
            x = ACTS[act](x)
    return x


def sigma_of(params):
    return params["std"] if "std" in params else torch.exp(params["log_std"])


def loss_terms(params, act, batch, hyper):
    """ppo.py:266-335 on one mini-batch: (loss, dict of the four means, per-row ratio, per-row value difference)."""
    mu = mlp(params, "actor", batch["observations"], act)
    sigma = sigma_of(params).expand_as(mu)
    value = mlp(params, "critic", batch["critic_observations"], act)
    logp = (-((batch["actions"] - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - LOG_SQRT_2PI).sum(-1)
    entropy = (0.5 + LOG_SQRT_2PI + torch.log(sigma)).sum(-1)
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / batch["sigma"] + 1.0e-5) + (batch["sigma"] ** 2 + (batch["mu"] - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, dim=-1).mean()
    adv = batch["advantages"].squeeze(-1)
    ratio = torch.exp(logp - batch["actions_log_prob"].squeeze(-1))
    c = hyper["clip_param"]
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)).mean()
    if hyper["use_clipped_value_loss"]:
        clipped = batch["values"] + (value - batch["values"]).clamp(-c, c)
        value_loss = torch.max((value - batch["returns"]).pow(2), (clipped - batch["returns"]).pow(2)).mean()
    else:
        value_loss = (batch["returns"] - value).pow(2).mean()
    loss = surrogate + hyper["value_loss_coef"] * value_loss - hyper["entropy_coef"] * entropy.mean()
    means = dict(surrogate=surrogate.detach(), value_function=value_loss.detach(), entropy=entropy.mean().detach(), kl=kl)
    return loss, means, ratio.detach(), (value - batch["values"]).detach().squeeze(-1)


def cast(tensors, dtype):
    return {k: v.detach().to(dtype).clone() for k, v in tensors.items()}


def gradients(params, act, batch, hyper, dtype=torch.float64):
    """Pre-clip gradients of one mini-batch in `dtype`: (dict of gradients, global norm, dict of loss means, ratio, value difference)."""
    p = {k: v.requires_grad_(True) for k, v in cast(params, dtype).items()}
    loss, means, ratio, dv = loss_terms(p, act, cast(batch, dtype), hyper)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in p.items()}
    norm = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
    return grads, norm, means, ratio, dv


def adaptive_learning_rate(lr, kl, desired_kl):
    """ppo.py:301-304."""
    if kl > desired_kl * 2.0:
        return max(1e-5, lr / 1.5)
    if kl < desired_kl / 2.0 and kl > 0.0:
        return min(1e-2, lr * 1.5)
    return lr


def fresh_state(params, dtype=torch.float64):
    return dict(exp_avg={k: torch.zeros_like(v, dtype=dtype) for k, v in params.items()},
                exp_avg_sq={k: torch.zeros_like(v, dtype=dtype) for k, v in params.items()}, step=0)


def clip_and_adam(params, grads, state, lr, max_grad_norm, dtype=torch.float64):
    """`clip_grad_norm_` then one `torch.optim.Adam` step (betas 0.9 / 0.999, eps 1e-8, no weight decay), out of place, in `dtype`."""
    g = cast(grads, dtype)
    norm = torch.sqrt(sum((x ** 2).sum() for x in g.values()))
    coef = torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0)
    step = state["step"] + 1
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    new_p, new_m, new_v = {}, {}, {}
    for k in params:
        gk = g[k] * coef
        m = state["exp_avg"][k].to(dtype) * 0.9 + 0.1 * gk
        v = state["exp_avg_sq"][k].to(dtype) * 0.999 + 0.001 * gk * gk
        new_p[k] = params[k].to(dtype) - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + 1e-8)
        new_m[k], new_v[k] = m, v
    return new_p, dict(exp_avg=new_m, exp_avg_sq=new_v, step=step)


def take(rows, idx):
    return {k: rows[k][idx] for k in ROW_KEYS}


def update(params, act, rows, perm, hyper, num_learning_epochs, num_mini_batches, learning_rate, dtype=torch.float64, state=None):
    """The whole `PPO.update`: returns (params, loss dict, final learning rate, trace) -- trace: per optimiser step the learning rate after the rule,
    the KL, the ratio rows and the value-difference rows.  Loss means are summed as Python floats, as the reference sums `.item()`s."""
    params = cast(params, dtype)
    rows = cast({k: rows[k] for k in ROW_KEYS}, dtype)
    state = state if state is not None else fresh_state(params, dtype)
    R = rows["observations"].shape[0]
    mini = R // num_mini_batches
    lr = learning_rate
    sums = dict(value_function=0.0, surrogate=0.0, entropy=0.0)
    trace = []
    for _ in range(num_learning_epochs):
        for i in range(num_mini_batches):
            batch = take(rows, perm[i * mini:(i + 1) * mini])
            grads, norm, means, ratio, dv = gradients(params, act, batch, hyper, dtype)
            if hyper["schedule"] == "adaptive":
                lr = adaptive_learning_rate(lr, float(means["kl"]), hyper["desired_kl"])
            params, state = clip_and_adam(params, grads, state, lr, hyper["max_grad_norm"], dtype)
            for k in sums:
                sums[k] += float(means[k])
            trace.append(dict(learning_rate=lr, kl=float(means["kl"]), ratio=ratio, dv=dv, norm=float(norm)))
    n = num_learning_epochs * num_mini_batches
    return params, {k: v / n for k, v in sums.items()}, lr, trace, state


def craft_rows(params, act, R, seed, kl_scale=0.05, ratio_spread=0.35, value_spread=0.3, share_observations=False):
    """Seeded float32 rows around the CURRENT policy that populate every branch of the clipped losses at the first step: the stored log-probs put
    the ratio at exp(ratio_spread * N(0, 1)) (about a quarter of the rows on each side of a 0.2 clip), the stored values sit value_spread * N(0, 1)
    from the critic's, the stored means / sigmas sit kl_scale away (the KL to the collection policy), the advantages are normalised."""
    g = torch.Generator().manual_seed(seed)
    p = cast(params, torch.float32)
    O, Oc = p[f"actor.{layer_names(p, 'actor')[0]}.weight"].shape[1], p[f"critic.{layer_names(p, 'critic')[0]}.weight"].shape[1]
    obs = torch.randn(R, O, generator=g)
    cobs = obs if share_observations and O == Oc else torch.randn(R, Oc, generator=g)
    with torch.no_grad():
        mu_now = mlp(p, "actor", obs, act)
        sigma_now = sigma_of(p).expand_as(mu_now)
        mu = mu_now + kl_scale * sigma_now * torch.randn(mu_now.shape, generator=g)
        sigma = (sigma_now * (1.0 + 0.5 * kl_scale)).contiguous()
        actions = mu + sigma * torch.randn(mu_now.shape, generator=g)
        logp_now = (-((actions - mu_now) ** 2) / (2 * sigma_now ** 2) - torch.log(sigma_now) - LOG_SQRT_2PI).sum(-1, keepdim=True)
        logp = logp_now - ratio_spread * torch.randn(R, 1, generator=g)
        values = mlp(p, "critic", cobs, act) + value_spread * torch.randn(R, 1, generator=g)
        returns = values + torch.randn(R, 1, generator=g)
        adv = torch.randn(R, 1, generator=g)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return dict(observations=obs, critic_observations=cobs, actions=actions, values=values, returns=returns, advantages=adv, actions_log_prob=logp,
                mu=mu, sigma=sigma)


def branch_fractions(ratio, dv, adv, clip):
    """Fractions of rows in each branch of the clipped losses: for each sign of the advantage the ratio below / inside / above the clip, and the value
    difference below / above the value clip."""
    out = {}
    for sign, mask in (("pos", adv > 0), ("neg", adv < 0)):
        out[sign + "_below"] = float((mask & (ratio < 1 - clip)).double().mean())
        out[sign + "_inside"] = float((mask & (ratio >= 1 - clip) & (ratio <= 1 + clip)).double().mean())
        out[sign + "_above"] = float((mask & (ratio > 1 + clip)).double().mean())
    out["value_below"], out["value_above"] = float((dv < -clip).double().mean()), float((dv > clip).double().mean())
    out["value_inside"] = 1.0 - out["value_below"] - out["value_above"]
    return out


def load_golden_case(name):
    """A case of tests/golden/ppo_update.npz (tools/refgen/make_ppo_update_golden.py): the state dict before (`sd0`, stored as float16, exact) and after
    (`sd1`) the reference's `PPO.update`, the storage rows, the permutation, the loss dict, the final learning rate and the settings."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_update.npz"))
    part = lambda tag: {k[len(name) + len(tag) + 2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(f"{name}.{tag}.")}  # noqa: E731
    cfg = json.loads(str(z[f"{name}.config"]))
    loss = dict(zip(("value_function", "surrogate", "entropy"), [float(x) for x in z[f"{name}.loss"]]))
    return dict(sd0=part("sd0"), sd1=part("sd1"), rows=part("rows"), perm=torch.from_numpy(z[f"{name}.perm"]), loss=loss,
                learning_rate=float(z[f"{name}.learning_rate"]), lr_trajectory=[float(x) for x in z[f"{name}.lr_trajectory"]], **cfg)

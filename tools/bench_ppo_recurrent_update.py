"""Native recurrent PPO update (rl.NativeRecurrentPPO, include/lgtrain_recurrent.h) against an eager-torch restatement of what the reference runs
(`ppo_update_recurrent` of tools/train_acceptance.py: `nn.LSTM` over the padded trajectories of the same dones, autograd, `optim.Adam`), interleaved
in one process, by the method of tools/bench_ppo_update.py.

Shapes: 4096 envs x 24 steps, LSTM 512 x 1 in front of [512, 256, 128], 5 epochs x 4 mini-batches, at 48 and 235 observations.  Synthetic rollout
rows; dones are drawn at the rate of a 1000-step episode plus one env in 64 done once more, so the padded block has pieces of every length.  Per
side: warm-up updates, then `--reps` timed updates, the sides alternating; HIP events around each update.  Records ms per update (median, min, max)
and per mini-batch for both, the launches per mini-batch of the native side (counted from the shapes: the kernels of one step are fixed), its
workspace bytes, the date and the library's hash.

usage: python tools/bench_ppo_recurrent_update.py [--reps 5] [--out profiles/ppo_recurrent_update.json]"""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def launches_per_mini_batch(T, layers, mlp_layers):
    """index + T x layers forward + MLP forward + loss (2) + MLP backward + dL/d(input) + T x layers backward + weight gradients, reduce, norm, Adam +
    the memory images."""
    return 1 + T * layers + 1 + 2 + (1 if mlp_layers > 1 else 0) + 1 + T * layers + 4 + 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_recurrent_update.json"))
    a = ap.parse_args(argv)
    from train_acceptance import ActorCriticRecurrent, ppo_update_recurrent
    from extended_legged_gym_amd.native import load_library
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
    T, N, A, E, M, H, L = 24, a.envs, 12, 5, 4, 512, 1
    alg = dict(num_learning_epochs=E, num_mini_batches=M, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, schedule="adaptive",
               desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True)
    results = []
    for name, O in (("flat_48", 48), ("rough_235", 235)):
        torch.manual_seed(0)
        ac = ActorCriticRecurrent(O, A, [512, 256, 128], [512, 256, 128], 1.0, "lstm", H, L).cuda()
        opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
        sd = {k: v.detach() for k, v in ac.state_dict().items()}
        nat = NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1)
        trainer = NativeRecurrentPPO(nat, sd, **alg)
        g = torch.Generator(device="cuda").manual_seed(1)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
        with torch.no_grad():
            obs = r(T, N, O)
            dones = (torch.rand(T, N, 1, device="cuda", generator=g) < 1e-3).float()
            dones[T // 2, ::64] = 1.0
            hid = [0.3 * r(T, L, N, H) for _ in range(4)]
            mu = 0.1 * r(T, N, A)
            sigma = ac.std.expand_as(mu).contiguous()
            act = mu + sigma * r(T, N, A)
            logp = torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True) + 0.1 * r(T, N, 1)
            val = 0.2 * r(T, N, 1)
        data = dict(observations=obs, actions=act, values=val, returns=val + r(T, N, 1), advantages=r(T, N, 1), actions_log_prob=logp, mu=mu, sigma=sigma,
                    dones=dones, hidden_states_a=(hid[0], hid[1]), hidden_states_c=(hid[2], hid[3]))
        times = {"native": [], "torch": []}
        lr = 1e-3
        for rep in range(a.warmup + a.reps):
            for side in ("native", "torch"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if side == "native":
                    trainer.update(data)
                else:
                    lr, _ = ppo_update_recurrent(ac, opt, data, alg, lr)
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[side].append(e0.elapsed_time(e1))
        row = dict(shape=name, num_obs=O, envs=N, steps=T, epochs=E, mini_batches=M, rnn="lstm", rnn_hidden=H, rnn_layers=L, rows_per_mini_batch=T * (N // M),
                   dones_fraction=float(dones.mean()), native_launches_per_mini_batch=launches_per_mini_batch(T, L, 4), native_workspace_bytes=trainer.workspace_bytes())
        for side, ts in times.items():
            med = statistics.median(ts)
            row[side] = dict(ms_per_update_median=med, ms_per_update_min=min(ts), ms_per_update_max=max(ts), ms_per_mini_batch=med / (E * M), reps=len(ts))
        row["native_over_torch"] = row["native"]["ms_per_update_median"] / row["torch"]["ms_per_update_median"]
        print(json.dumps(row), flush=True)
        results.append(row)
        trainer.close()
    lib = load_library()
    digest = hashlib.sha256(open(lib._name, "rb").read()).hexdigest()[:16]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), library_sha256=digest, results=results), f, indent=1)


if __name__ == "__main__":
    main()

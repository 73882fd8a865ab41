"""Native PPO update (rl.NativePPO, include/lgtrain.h) against the eager-torch `ppo_update` of tools/train_acceptance.py, interleaved in one process.

Shapes: 4096 envs x 24 steps, 5 epochs x 4 mini-batches, at 48 observations (anymal_c_flat) and 235 (anymal_c_rough), networks 512-256-128, ELU.
Synthetic rollout rows (the update's cost does not depend on their values).  Per side and shape: warm-up updates, then `--reps` timed updates, the
two sides alternating; wall clock around a device synchronisation (the update is one enqueue on the native side; the torch side syncs per
mini-batch by itself).  Reports ms per update (median, min, max), ms per mini-batch, and TFLOP/s of the matrix work (forward 2, backward data 2,
weight gradient 2 FLOP per weight per row, no backward data into the observations) against the fp32 matrix peak.

usage: python tools/bench_ppo_update.py [--reps 7] [--out profiles/ppo_update.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FP32_MATRIX_PEAK_TFLOPS = 157.3          # MI355X, dense fp32 matrix


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update.json"))
    a = ap.parse_args(argv)
    from train_acceptance import ActorCritic, ppo_update
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    T, N, A, E, M = 24, 4096, 12, 5, 4
    alg = dict(num_learning_epochs=E, num_mini_batches=M, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, schedule="adaptive",
               desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True)
    results = []
    for name, O in (("flat_48", 48), ("rough_235", 235)):
        torch.manual_seed(0)
        ac = ActorCritic(O, A, [512, 256, 128], [512, 256, 128], 1.0).cuda()
        opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
        sd = {k: v.detach() for k, v in ac.state_dict().items()}
        nat = NativeActorCritic(sd, "elu", device="cuda:0", seed=1)
        trainer = NativePPO(nat, sd, **alg)
        g = torch.Generator(device="cuda").manual_seed(1)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
        with torch.no_grad():
            obs = r(T, N, O)
            mu = ac.actor(obs)
            sigma = ac.std.expand_as(mu).contiguous()
            act = mu + sigma * r(T, N, A)
            logp = torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True) + 0.1 * r(T, N, 1)
            val = ac.critic(obs) + 0.2 * r(T, N, 1)
        data = dict(observations=obs, actions=act, values=val, returns=val + r(T, N, 1), advantages=r(T, N, 1), actions_log_prob=logp, mu=mu, sigma=sigma)
        weights = sum(p.numel() for n_, p in ac.named_parameters() if n_.endswith("weight"))
        first = 2 * O * 512          # the two first layers: no backward data pass into the observations
        flop = E * M * (T * N // M) * 2.0 * (3 * weights - first)
        times = {"native": [], "torch": []}
        lr = 1e-3
        for rep in range(a.warmup + a.reps):
            for side in ("native", "torch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if side == "native":
                    trainer.update(data)
                else:
                    lr, _ = ppo_update(ac, opt, data, alg, lr)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[side].append((time.perf_counter() - t0) * 1e3)
        row = dict(shape=name, num_obs=O, envs=N, steps=T, epochs=E, mini_batches=M, rows_per_mini_batch=T * N // M, matrix_gflop_per_update=flop / 1e9)
        for side, ts in times.items():
            med = statistics.median(ts)
            row[side] = dict(ms_per_update_median=med, ms_per_update_min=min(ts), ms_per_update_max=max(ts), ms_per_mini_batch=med / (E * M),
                             tflops=flop / (med * 1e-3) / 1e12, fraction_of_fp32_matrix_peak=flop / (med * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TFLOPS, reps=len(ts))
        row["native_over_torch"] = row["native"]["ms_per_update_median"] / row["torch"]["ms_per_update_median"]
        print(json.dumps(row), flush=True)
        results.append(row)
        trainer.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), fp32_matrix_peak_tflops=FP32_MATRIX_PEAK_TFLOPS, results=results), f, indent=1)


if __name__ == "__main__":
    main()

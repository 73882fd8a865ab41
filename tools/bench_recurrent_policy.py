"""Recurrent policy step, informational (the method of tools/bench_rollout.py, HIP events): 4096 rows, obs 235, LSTM hidden 512 x 1 layer, MLP
[512, 256, 128].  (a) `lg_policy_act_recurrent` (both memories + both MLPs + sampling); (b) the same networks in eager PyTorch-ROCm, as rsl_rl's
`ActorCriticRecurrent.act` + `evaluate` run them (`nn.LSTM` on a one-step sequence, `nn.Sequential`, `torch.distributions.Normal`);
(c) for scale, the feed-forward `lg_policy_act` on 235 -> [512, 256, 128].  One JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from extended_legged_gym_amd.rl import NativeActorCritic, NativeActorCriticRecurrent  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12          # MI355X: 256 CUs x 4 SIMDs x 64 FLOP / cycle (v_mfma_f32_16x16x4_f32) x 2.4 GHz


def timeit(fn, warm=20, steps=100, repeats=5):
    """Median over `repeats` windows of `steps` calls between two HIP events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / steps)
    return sorted(times)[len(times) // 2], min(times), max(times)


def seq(dims):
    mods = []
    for a, b in zip(dims[:-2], dims[1:-1]):
        mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(dims[-2], dims[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rnn-type", default="lstm")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, O, H, L, A, mlp = args.rows, 235, args.hidden, args.layers, 12, [512, 256, 128]
    torch.manual_seed(0)
    cls = torch.nn.LSTM if args.rnn_type == "lstm" else torch.nn.GRU
    mem_a, mem_c = cls(O, H, L).cuda(), cls(O, H, L).cuda()
    actor, critic = seq([H] + mlp + [A]).cuda(), seq([H] + mlp + [1]).cuda()
    std = torch.ones(A, device="cuda")
    sd = {"std": std}
    for pre, m in (("memory_a.rnn.", mem_a), ("memory_c.rnn.", mem_c), ("actor.", actor), ("critic.", critic)):
        sd.update({pre + k: v for k, v in m.state_dict().items()})
    rec = NativeActorCriticRecurrent(sd, "elu", args.rnn_type, device="cuda:0", seed=1)
    ff_a, ff_c = seq([O] + mlp + [A]), seq([O] + mlp + [1])
    fsd = {"std": std}
    fsd.update({"actor." + k: v for k, v in ff_a.state_dict().items()})
    fsd.update({"critic." + k: v for k, v in ff_c.state_dict().items()})
    ff = NativeActorCritic(fsd, "elu", device="cuda:0", seed=1)
    obs = torch.randn(N, O, device="cuda")
    state = {"a": None, "c": None}

    def eager():                      # ActorCriticRecurrent.act + evaluate (actor_critic_recurrent.py:66-80) as PPO.act calls them (ppo.py:147-159)
        with torch.no_grad():
            oa, state["a"] = mem_a(obs.unsqueeze(0), state["a"])
            mean = actor(oa.squeeze(0))
            dist = torch.distributions.Normal(mean, std.expand_as(mean))
            a = dist.sample()
            oc, state["c"] = mem_c(obs.unsqueeze(0), state["c"])
            v = critic(oc.squeeze(0))
            lp = dist.log_prob(a).sum(-1)
        return a, v, lp

    G = 4 if args.rnn_type == "lstm" else 3
    mem_flops = 2.0 * N * G * H * sum((O if l == 0 else H) + H for l in range(L))
    mlp_flops = 2.0 * N * (H * 512 + 512 * 256 + 256 * 128) * 2 + 2.0 * N * 128 * (A + 1)
    flops = 2.0 * mem_flops + mlp_flops
    t_native = timeit(lambda: rec.act_and_evaluate(obs))
    t_eager = timeit(eager)
    t_ff = timeit(lambda: ff.act_and_evaluate(obs))
    t_mem = timeit(lambda: rec.memory_a(obs))
    lib = os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so")
    res = {"what": "recurrent policy step (PPO.act of an ActorCriticRecurrent)", "rows": N, "obs": O, "rnn_type": args.rnn_type, "hidden": H, "layers": L, "mlp": mlp,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "date": time.strftime("%Y-%m-%d"),
           "library_sha256": subprocess.run(["sha256sum", lib], capture_output=True, text=True).stdout.split()[0][:16],
           "native_act_recurrent_us": {"median": t_native[0] * 1e6, "min": t_native[1] * 1e6, "max": t_native[2] * 1e6},
           "eager_torch_act_evaluate_us": {"median": t_eager[0] * 1e6, "min": t_eager[1] * 1e6, "max": t_eager[2] * 1e6},
           "native_feed_forward_act_us": {"median": t_ff[0] * 1e6, "min": t_ff[1] * 1e6, "max": t_ff[2] * 1e6},
           "one_memory_step_us": {"median": t_mem[0] * 1e6, "min": t_mem[1] * 1e6, "max": t_mem[2] * 1e6},
           "speedup_vs_eager": t_eager[0] / t_native[0], "gflop_per_call": flops * 1e-9,
           "fraction_of_fp32_matrix_peak": flops / t_native[0] / FP32_MATRIX_PEAK,
           "one_memory_fraction_of_fp32_matrix_peak": mem_flops / t_mem[0] / FP32_MATRIX_PEAK,
           "timing": "HIP events around 100 back-to-back calls, median / min / max of 5 windows after 20 warm-up calls (host enqueue included)"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

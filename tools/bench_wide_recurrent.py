"""The recurrent policy on the 578-wide row (lg_rnn_create_wide: input projection + seeded step), by the protocol of tools/bench_recurrent_policy.py
and tools/bench_ppo_recurrent_update.py: every comparison in one process, the sides alternating block by block, median [min, max] over the blocks,
the date and the library's hash in the file.

  act      `lg_policy_act_recurrent` at 4096 rows, 578 -> LSTM / GRU 512 x 1 -> 512-256-128 -> 18, against eager torch (`nn.LSTM` / `nn.GRU` on a one-step
           sequence + the MLPs + `Normal`).  HIP events around 100 back-to-back calls per block.
  update   `NativeRecurrentPPO.update` at 4096 envs x 24 steps, 5 epochs x 4 mini-batches, the same network (LSTM), against eager torch over padded
           trajectories (`ppo_update_recurrent` of tools/train_acceptance.py).  Reported, not gated.
  narrow   with `--parent-lib PATH` (the library built from the parent commit): the act and the update at 235 columns through both libraries in
           alternating blocks; `inside_parent_spread` says whether the new median lies within the parent's own min .. max.
  runner   one `NativeOnPolicyRunner` iteration (`learn(1)`) on elspider_air_rough_raycast with the recurrent policy, `sensor_collection` host and native.
  share    `--kernel-stats CSV` (the kernel statistics of a kernel-trace run of `--mode trace`, a run of its own): the projection's share of the act.

usage: python tools/bench_wide_recurrent.py [--blocks 5] [--parent-lib PATH] [--kernel-stats CSV] [--out profiles/wide_recurrent.json]
       python tools/bench_wide_recurrent.py --mode trace          (200 acts per memory type and nothing else: the program a kernel trace wraps)"""
import argparse
import contextlib
import copy
import csv
import datetime
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS, WIDE, NARROW, H, A, MLP = 4096, 578, 235, 512, 18, [512, 256, 128]


@contextlib.contextmanager
def library(path):
    """The rl objects created inside bind to the library at `path` (each keeps the library it was created with)."""
    from extended_legged_gym_amd import abi, native
    keep = (native._lib, native.LIB_PATH, abi.UNITS["policy_wide"])

    def tolerant(lib):          # the parent's library has no wide-memory entry points
        try:
            return keep[2].declare(lib)
        except AttributeError:
            return lib
    native._lib, native.LIB_PATH, abi.UNITS["policy_wide"] = None, path, keep[2]._replace(declare=tolerant)
    try:
        yield
    finally:
        native._lib, native.LIB_PATH, abi.UNITS["policy_wide"] = keep


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), blocks=list(xs))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls          # ms per call


def interleaved(sides, blocks, calls, warm):
    """sides: name -> callable.  One warm-up block each, then `blocks` rounds in which every side runs one window."""
    for fn in sides.values():
        window(fn, warm)
    out = {name: [] for name in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            out[name].append(window(fn, calls))
    return {name: spread(v) for name, v in out.items()}


def seq(dims):
    mods = []
    for a, b in zip(dims[:-2], dims[1:-1]):
        mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(dims[-2], dims[-1]))


def act_network(rnn_type, O):
    torch.manual_seed(0)
    cls = torch.nn.LSTM if rnn_type == "lstm" else torch.nn.GRU
    mods = dict(mem_a=cls(O, H, 1).cuda(), mem_c=cls(O, H, 1).cuda(), actor=seq([H] + MLP + [A]).cuda(), critic=seq([H] + MLP + [1]).cuda())
    sd = {"std": torch.ones(A, device="cuda")}
    for pre, m in (("memory_a.rnn.", mods["mem_a"]), ("memory_c.rnn.", mods["mem_c"]), ("actor.", mods["actor"]), ("critic.", mods["critic"])):
        sd.update({pre + k: v.detach() for k, v in m.state_dict().items()})
    return mods, sd


def eager_act(mods, obs, std):
    state = {"a": None, "c": None}

    def fn():          # ActorCriticRecurrent.act + evaluate as PPO.act calls them
        with torch.no_grad():
            oa, state["a"] = mods["mem_a"](obs.unsqueeze(0), state["a"])
            mean = mods["actor"](oa.squeeze(0))
            dist = torch.distributions.Normal(mean, std.expand_as(mean))
            a = dist.sample()
            oc, state["c"] = mods["mem_c"](obs.unsqueeze(0), state["c"])
            return a, mods["critic"](oc.squeeze(0)), dist.log_prob(a).sum(-1)
    return fn


def bench_act(blocks):
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    rows = []
    for rnn_type in ("lstm", "gru"):
        mods, sd = act_network(rnn_type, WIDE)
        nat = NativeActorCriticRecurrent(sd, "elu", rnn_type, device="cuda:0", seed=1)
        obs = torch.randn(ROWS, WIDE, device="cuda")
        r = interleaved({"native": lambda: nat.act_and_evaluate(obs), "torch": eager_act(mods, obs, sd["std"])}, blocks, 100, 20)
        row = dict(what="lg_policy_act_recurrent", rows=ROWS, num_obs=WIDE, rnn=rnn_type, rnn_hidden=H, mlp=MLP, actions=A, native_ms=r["native"], torch_ms=r["torch"],
                   torch_over_native=r["torch"]["median"] / r["native"]["median"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def update_case(O):
    from train_acceptance import ActorCriticRecurrent
    T, N, L = 24, ROWS, 1
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(O, A, MLP, MLP, 1.0, "lstm", H, L).cuda()
    sd = {k: v.detach().clone() for k, v in ac.state_dict().items()}
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
    return ac, sd, data


ALG = dict(num_learning_epochs=5, num_mini_batches=4, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, schedule="adaptive",
           desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True)


def bench_update(blocks):
    from train_acceptance import ppo_update_recurrent
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
    ac, sd, data = update_case(WIDE)
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    trainer = NativeRecurrentPPO(NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1), sd, **ALG)
    lr = [1e-3]

    def eager():
        lr[0], _ = ppo_update_recurrent(ac, opt, data, ALG, lr[0])
    r = interleaved({"native": lambda: trainer.update(data), "torch": eager}, blocks, 1, 1)
    row = dict(what="NativeRecurrentPPO.update", num_obs=WIDE, envs=ROWS, steps=24, epochs=5, mini_batches=4, rnn="lstm", rnn_hidden=H, mlp=MLP,
               native_ms=r["native"], torch_ms=r["torch"], native_over_torch=r["native"]["median"] / r["torch"]["median"],
               native_workspace_bytes=trainer.workspace_bytes())
    print(json.dumps(row), flush=True)
    trainer.close()
    return row


def bench_narrow(blocks, parent_lib):
    """The 235-column act and update through this build and through the parent commit's library, alternating."""
    from extended_legged_gym_amd import native
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
    rows = []
    _, sd = act_network("lstm", NARROW)
    obs = torch.randn(ROWS, NARROW, device="cuda")
    new = NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1)
    with library(parent_lib):
        old = NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1)
    assert old.actor.lib is not new.actor.lib
    a, b = new.act_and_evaluate(obs), old.act_and_evaluate(obs)
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    r = interleaved({"parent": lambda: old.act_and_evaluate(obs), "new": lambda: new.act_and_evaluate(obs)}, blocks, 100, 20)
    rows.append(dict(what="lg_policy_act_recurrent", num_obs=NARROW, rows=ROWS, parent_ms=r["parent"], new_ms=r["new"], equal_bits=same,
                     inside_parent_spread=r["parent"]["min"] <= r["new"]["median"] <= r["parent"]["max"]))
    print(json.dumps(rows[-1]), flush=True)
    _, sd, data = update_case(NARROW)
    tn = NativeRecurrentPPO(NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1), sd, **ALG)
    with library(parent_lib):
        to = NativeRecurrentPPO(NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1), sd, **ALG)
    # one update each on trainers of their own: this build twice (its own determinism at this size) and the parent's once
    first = []
    for lib_path in (None, None, parent_lib):
        with library(lib_path) if lib_path else contextlib.nullcontext():
            t = NativeRecurrentPPO(NativeActorCriticRecurrent(sd, "elu", "lstm", device="cuda:0", seed=1), sd, **ALG)
        t.update(data)
        first.append(t.state_dict())
        t.close()
    one_update = dict(new_equals_new=all(torch.equal(first[0][k], first[1][k]) for k in first[0]),
                      new_equals_parent=all(torch.equal(first[0][k], first[2][k]) for k in first[0]))
    print(json.dumps(one_update), flush=True)
    r = interleaved({"parent": lambda: to.update(data), "new": lambda: tn.update(data)}, blocks, 1, 1)
    pa, pb = to.state_dict(), tn.state_dict()
    rows.append(dict(what="NativeRecurrentPPO.update", num_obs=NARROW, envs=ROWS, steps=24, epochs=5, mini_batches=4, parent_ms=r["parent"], new_ms=r["new"],
                     equal_bits=all(torch.equal(pa[k], pb[k]) for k in pa), equal_bits_after_one_update=one_update,
                     inside_parent_spread=r["parent"]["min"] <= r["new"]["median"] <= r["parent"]["max"]))
    print(json.dumps(rows[-1]), flush=True)
    to.close(); tn.close()
    return dict(parent_library_sha256=hashlib.sha256(open(parent_lib, "rb").read()).hexdigest()[:16], rows=rows,
                rule="the new build passes if its median lies inside the parent's own block spread (min .. max)")


def bench_runner(blocks, envs, steps):
    from train_estimator import make_env
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import NativeOnPolicyRunner
    from extended_legged_gym_amd.utils.helpers import class_to_dict
    task = "elspider_air_rough_raycast"
    cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(task)[1]))
    cfg["runner"].update(num_steps_per_env=steps, policy_class_name="ActorCriticRecurrent")
    cfg["policy"].pop("class_name", None)
    cfg["policy"].update(rnn_hidden_size=H, rnn_type="lstm", rnn_num_layers=1, actor_hidden_dims=MLP, critic_hidden_dims=MLP)
    runners = {}
    for how in ("host", "native"):
        c = copy.deepcopy(cfg)
        c["runner"]["sensor_collection"] = how
        runners[how] = NativeOnPolicyRunner(make_env(envs), c, log_dir=None, device="cuda:0")
        runners[how].learn(1)          # warm-up: code objects, allocations, the carried rows, the rig
    ts = {how: [] for how in runners}
    for _ in range(blocks):
        for how, runner in runners.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.learn(1)
            torch.cuda.synchronize()
            ts[how].append((time.perf_counter() - t0) * 1e3)
    out = {how: spread(v) for how, v in ts.items()}
    print(json.dumps({"runner_ms_per_iteration": out}), flush=True)
    return dict(what="one NativeOnPolicyRunner iteration (collection + update), wall clock", task=task, envs=envs, steps=steps, policy="ActorCriticRecurrent lstm 512 x 1",
                ms_per_iteration=out)


def projection_share(path):
    """Kernel statistics of a kernel-trace run of `--mode trace`: the share of the recurrent act's kernels that the projection takes."""
    total, by = 0.0, {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0)
        for key in ("rnn_wide_xproj_kernel", "rnn_wide_layer_kernel", "policy_act_kernel"):
            if key in name:
                by[key] = by.get(key, 0.0) + ns
                total += ns
    return dict(source=os.path.basename(path), kernel_ns=by, projection_share_of_the_act=by.get("rnn_wide_xproj_kernel", 0.0) / total if total else None)


def trace_program():
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    for rnn_type in ("lstm", "gru"):
        _, sd = act_network(rnn_type, WIDE)
        nat = NativeActorCriticRecurrent(sd, "elu", rnn_type, device="cuda:0", seed=1)
        obs = torch.randn(ROWS, WIDE, device="cuda")
        for _ in range(200):
            nat.act_and_evaluate(obs)
        torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("bench", "trace"), default="bench")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--runner-envs", type=int, default=4096)
    ap.add_argument("--runner-steps", type=int, default=24)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out: act,update,narrow,runner")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_recurrent.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_recurrent needs the GPU: a CPU run has no timing to give")
    if a.mode == "trace":
        return trace_program()
    from extended_legged_gym_amd.native import load_library
    skip = set(filter(None, a.skip.split(",")))
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, date=datetime.date.today().isoformat(),
               library_sha256=hashlib.sha256(open(load_library()._name, "rb").read()).hexdigest()[:16],
               timing="interleaved blocks in one process; ms; median [min, max] over the blocks; act: HIP events around 100 back-to-back calls per block, "
                      "update: HIP events around one update per block, runner: wall clock around learn(1)")
    if os.path.exists(a.out):          # sections measured in an earlier run of their own stay
        old = json.load(open(a.out))
        res.update({k: v for k, v in old.items() if k in ("act", "update", "narrow_path", "runner", "projection")})
    if "act" not in skip:
        res["act"] = bench_act(a.blocks)
    if "update" not in skip:
        res["update"] = bench_update(a.blocks)
    if a.parent_lib and "narrow" not in skip:
        res["narrow_path"] = bench_narrow(a.blocks, a.parent_lib)
    if "runner" not in skip:
        res["runner"] = bench_runner(a.blocks, a.runner_envs, a.runner_steps)
    if a.kernel_stats:
        res["projection"] = projection_share(a.kernel_stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""`collect_rollout`: the data-collection loop of `OnPolicyRunner.learn` (`rsl_rl/runners/on_policy_runner.py:395-445`:
`PPO.act` -> `env.step` -> `PPO.process_env_step`, `num_steps_per_env` times, then `PPO.compute_returns`) as ONE call
into the library (`lg_collect_rollout`, include/lgpolicy.h).  The host enqueues the whole rollout and returns; the rows
come back as the tensors `RolloutStorage` holds (`storage/rollout_storage.py:47-76`).  A recurrent policy (`policy.is_recurrent`) goes through
`lg_collect_rollout_recurrent`, which also keeps the hidden-state rows of `RolloutStorage._save_hidden_states` (`:123-140`)."""
import ctypes as C

import torch

from extended_legged_gym_amd import abi
from .policy import _check, _lib, _ptr


def empty(device, *shape):
    """An uninitialised float32 tensor: every row of a collection is written before it is read."""
    return torch.empty(*shape, device=device, dtype=torch.float32)


def _advance(env, policy, T):
    """What a collection of T steps leaves behind on the host side: T sampling calls drawn, T env steps counted."""
    policy._call += T
    if hasattr(env, "common_step_counter"):
        env.common_step_counter += T


def collect_rollout(env, policy, num_steps, gamma=0.99, lam=0.95, normalize_advantage=True, compute_returns=True):
    """env: a native `LeggedRobot` (its `core` holds the context); policy: `NativeActorCritic` or `NativeActorCriticRecurrent`.  Returns a
    dict of (T, N, .) tensors: observations, actions, rewards, dones, values, actions_log_prob, mu, sigma, returns, advantages
    (+ last_values (N, 1)).  Draws the same samples as `num_steps` calls of `policy.act_and_evaluate`.
    Recurrent policy: also `hidden_states_a` / `hidden_states_c`, the state of each memory BEFORE step t's act (`ppo.py:148-149`), (T, L, N, H)
    -- a tuple `(h, c)` for an LSTM; the memories are reset on `dones[t]` after each step (`ppo.py:188`), and `last_values` advances the critic
    memory once more, as `policy.evaluate` does in the reference (`ppo.py:190-192`)."""
    lib = _lib()
    dev = policy.device
    T, N, O, A = int(num_steps), env.core.t["obs_buf"].shape[0], env.core.t["obs_buf"].shape[1], policy.num_actions
    out, rows = rollout_rows(T, N, O, A, dev, compute_returns)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (_ptr(policy.std), policy.seed, policy._call + 1, T, float(gamma), float(lam), int(bool(normalize_advantage)), C.byref(rows))
    if not getattr(policy, "is_recurrent", False):
        _check(lib.lg_collect_rollout(env.core.ctx, policy.actor.handle, policy.critic.handle, *head, stream), "lg_collect_rollout")
    else:
        mems, hidden, state, stacks = _hidden_rows(policy, T, N)
        _check(lib.lg_collect_rollout_recurrent(env.core.ctx, mems[0], policy.actor.handle, mems[1], policy.critic.handle, *head, C.byref(hidden), *state, stream),
               "lg_collect_rollout_recurrent")
        out.update(stacks)
    _advance(env, policy, T)
    return out


def rollout_rows(T, N, O, A, dev, compute_returns=True):
    """The (T, N, .) tensors of one PPO collection (`observations` O wide) and the `abi.lg_rollout` over them."""
    out = dict(observations=empty(dev, T, N, O), actions=empty(dev, T, N, A), rewards=empty(dev, T, N, 1), dones=empty(dev, T, N, 1), values=empty(dev, T, N, 1),
               actions_log_prob=empty(dev, T, N, 1), mu=empty(dev, T, N, A), sigma=empty(dev, T, N, A), last_values=empty(dev, N, 1))
    if compute_returns:
        out.update(returns=empty(dev, T, N, 1), advantages=empty(dev, T, N, 1))
    return out, abi.lg_rollout(**{k: v.data_ptr() for k, v in out.items()})


def _hidden_rows(policy, T, N):
    """What a recurrent collection passes beyond a feed-forward one: the two memory handles, the `abi.lg_rollout_hidden` over fresh (T, L, N, H)
    stacks, the live state pointers (h_a, c_a, h_c, c_c), and the stacks as the dict's `hidden_states_a` / `hidden_states_c` (`(h, c)` for an LSTM)."""
    mems = (policy.memory_a, policy.memory_c)
    stacks = []
    for m in mems:
        m.ensure_state(N)
        stacks.append([torch.empty(T, m.num_layers, N, m.hidden_size, device=policy.device) for _ in range(2 if m.rnn_type == "lstm" else 1)])
    ptr = [[s.data_ptr() for s in st] + [None] * (2 - len(st)) for st in stacks]
    hidden = abi.lg_rollout_hidden(h_a=ptr[0][0], c_a=ptr[0][1], h_c=ptr[1][0], c_c=ptr[1][1])
    keys = {"hidden_states_" + k: tuple(st) if len(st) == 2 else st[0] for k, st in zip("ac", stacks)}
    return (mems[0].handle, mems[1].handle), hidden, (*mems[0]._ptrs(), *mems[1]._ptrs()), keys


class EpisodeTracker:
    """The live sums of the runner's episode bookkeeping (`on_policy_runner.py:372-373`), (N) float32 on the device, and the two 100-deep buffers
    (`:370-371`).  `collect_rollout_tracked(..., episode_tracker=...)` and `track` update the sums in place; `extend` takes a collection's finished
    episodes in the reference's `extend` order ((t, env): `dones.nonzero()`), with one device-to-host copy."""

    def __init__(self, num_envs, device="cuda:0", maxlen=100):
        from collections import deque
        self.device = torch.device(device)
        self.cur_reward_sum = torch.zeros(int(num_envs), device=self.device)
        self.cur_episode_length = torch.zeros(int(num_envs), device=self.device)
        self.rewbuffer, self.lenbuffer = deque(maxlen=maxlen), deque(maxlen=maxlen)

    def track(self, rewards, dones):
        """`lg_runner_episode_track` (include/lgrunner.h) over (T, N) rows: per env `sum += r; len += 1; if done: emit and zero`.  Returns
        (ep_return, ep_length), (T, N), defined where `dones > 0` (0 elsewhere)."""
        from .normalizer import _runner_lib
        r = rewards.to(self.device, torch.float32).reshape(rewards.shape[0], -1).contiguous()
        d = dones.to(self.device, torch.float32).reshape(dones.shape[0], -1).contiguous()
        assert r.shape == d.shape and r.shape[1] == self.cur_reward_sum.shape[0]
        ep_return, ep_length = torch.empty_like(r), torch.empty_like(r)
        _check(_runner_lib().lg_runner_episode_track(_ptr(r), _ptr(d), r.shape[0], r.shape[1], _ptr(self.cur_reward_sum), _ptr(self.cur_episode_length),
                                                     _ptr(ep_return), _ptr(ep_length), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
               "lg_runner_episode_track")
        return ep_return, ep_length

    def extend(self, dones, ep_return, ep_length):
        done = dones.reshape(ep_return.shape) > 0
        both = torch.stack([ep_return[done], ep_length[done]]).cpu().numpy()
        self.rewbuffer.extend(both[0].tolist())
        self.lenbuffer.extend(both[1].tolist())


def _one_mode(obs_normalizer, privileged_obs_normalizer):
    """The `training` flag of a call with up to two normalisers: one mode for both handles (the reference keeps the second in training mode
    with the first, `on_policy_runner.py:736-738`), the only one's when there is one, 0 without any."""
    norms = [n for n in (obs_normalizer, privileged_obs_normalizer) if n is not None]
    if len(norms) == 2 and bool(norms[0].training) != bool(norms[1].training):
        raise ValueError("obs_normalizer and privileged_obs_normalizer are in different modes")
    return int(bool(norms[0].training)) if norms else 0


def _episode_hook(hooks, env, episode_tracker, T, N, dev):
    """Points `hooks.episode` at an `abi.lg_runner_episode` over fresh `raw_rewards` (T, N, 1), `episode_extras` (T, K), `ep_return` /
    `ep_length` (T, N, 1) and the tracker's live sums, and returns the four tensors by name.  No tracker: nothing."""
    if episode_tracker is None:
        return {}
    extra = dict(raw_rewards=empty(dev, T, N, 1), episode_extras=empty(dev, T, env.core.t["extras_episode"].numel()), ep_return=empty(dev, T, N, 1),
                 ep_length=empty(dev, T, N, 1))
    assert episode_tracker.cur_reward_sum.shape == (N,) and episode_tracker.cur_reward_sum.device == extra["raw_rewards"].device
    hooks.episode = C.pointer(abi.lg_runner_episode(raw_rewards=extra["raw_rewards"].data_ptr(), extras=extra["episode_extras"].data_ptr(),
                                                    cur_reward_sum=episode_tracker.cur_reward_sum.data_ptr(),
                                                    cur_episode_length=episode_tracker.cur_episode_length.data_ptr(),
                                                    ep_return=extra["ep_return"].data_ptr(), ep_length=extra["ep_length"].data_ptr()))
    return extra


def collect_rollout_tracked(env, policy, num_steps, gamma=0.99, lam=0.95, normalize_advantage=True, compute_returns=True, obs_normalizer=None,
                            episode_tracker=None, privileged_obs_normalizer=None, noise_uniforms=None, actor_columns=None, sensors=None):
    """`collect_rollout` through `lg_runner_collect` (include/lgrunner.h), with the runner's two device pieces between the launches of the one
    call.  Same dict; both hooks None: the same rows, bit for bit.
    obs_normalizer (`NativeEmpiricalNormalization`): every new observation row is normalised in place (and counted when the normaliser is in
    training mode) before it is stored and before the next act (`on_policy_runner.py:425-427`); row 0 is the normaliser's carried row -- the
    normalised row after the previous collection's last step -- or, when it holds none, the env's raw observation, as the first observation of
    `learn()` (`:364-365`); `last_values` is evaluated on the new carried row.  `env.obs_buf` stays raw.
    episode_tracker (`EpisodeTracker`): adds `raw_rewards` (T, N, 1), the env's reward without the time-out bootstrap `rewards` carries,
    `episode_extras` (T, K), the env's `extras_episode` tensor after each step, and `ep_return` / `ep_length` (T, N, 1), defined where
    `dones > 0`; the tracker's live sums advance in place (its buffers do not: `episode_tracker.extend(...)`).

    PRIVILEGED CRITIC OBSERVATIONS (`lg_runner_collect_privileged`, include/lgrunner_privileged.h: the library's one PPO collection loop in its
    two-stream mode; everything above holds, per stream): an env with an observation history
    (`env.obs_history`, (N, H, W): `AnymalStudent`), or `actor_columns=k` on any env (the actor reads the first k columns of the env's row).  The
    critic reads the env's own row (O_c wide), the actor the history's row (H * W) or the prefix; the dict then holds `observations` (T, N, O_a) and
    also `privileged_observations` (T, N, O_c), `values` are the critic's on the privileged rows.  `obs_normalizer` is the ACTOR's,
    `privileged_obs_normalizer` the critic's: each with its own carried row.  The history is stepped in place by the library and `env.obs_buf` is
    left as the actor's un-normalised row after the last step, as `collect_distillation` does; noise follows `env.add_noise`, and `noise_uniforms`
    (T, N, H * W) replaces the Philox draws.  For every other env the three arguments must stay None and the call is the one above.

    SENSORS (`lg_runner_collect_sensors`, include/lgsensors.h): `sensors`, a `SensorRig` of this env (`rl/sensors.py`), for an env whose step
    drives the ray caster and the depth camera (`LeggedRobotRayCast`, `LeggedRobotDepth`): every step of the call is the library's sensor step,
    the rows are those of a host loop over `env.step`, and the env's sensors and counters are left as that loop leaves them.  One stream only."""
    from .normalizer import _runner_lib
    lib = _runner_lib()
    if sensors is not None:
        from .sensors import _sensor_lib
        lib = _sensor_lib()
        if sensors.env is not env:
            raise ValueError("sensors: the rig belongs to another env")
    dev = policy.device
    T, N, O, A = int(num_steps), env.core.t["obs_buf"].shape[0], env.core.t["obs_buf"].shape[1], policy.num_actions
    hist = getattr(env, "obs_history", None)
    privileged = hist is not None or actor_columns is not None
    if privileged and sensors is not None:
        raise ValueError("sensors: a sensor rig together with privileged observations (an observation history, actor_columns) is not built")
    if not privileged and (privileged_obs_normalizer is not None or noise_uniforms is not None):
        raise ValueError("privileged_obs_normalizer / noise_uniforms need an env with an observation history, or actor_columns")
    O_c = O
    if privileged:
        rec = getattr(policy, "is_recurrent", False)
        O = policy.memory_a.input_size if rec else policy.actor.dims[0]
        if actor_columns is not None and (hist is not None or int(actor_columns) != O):
            raise ValueError(f"actor_columns = {actor_columns}: the actor reads {O} columns" + (", and the env has an observation history" if hist is not None else ""))
    out, rows = rollout_rows(T, N, O, A, dev, compute_returns)
    if obs_normalizer is not None and obs_normalizer.num_features != O:
        raise ValueError(f"the normaliser holds {obs_normalizer.num_features} columns, the env's observations {O}")
    hooks = abi.lg_runner_hooks(normalizer=obs_normalizer.handle if obs_normalizer is not None else None,
                                training=_one_mode(obs_normalizer, privileged_obs_normalizer))
    extra = _episode_hook(hooks, env, episode_tracker, T, N, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (_ptr(policy.std), policy.seed, policy._call + 1, T, float(gamma), float(lam), int(bool(normalize_advantage)), C.byref(rows))
    call, name, tail, last, keep = lib.lg_runner_collect, "lg_runner_collect", (), None, []
    if privileged:          # the second stream: its rows, the actor's layer and the critic's normaliser ride in one more struct
        crit = privileged_obs_normalizer          # (its width is the library's to check, with every other width of the call)
        out["privileged_observations"] = empty(dev, T, N, O_c)
        layer = None
        if hist is not None:
            last = empty(dev, N, O)
            layer, keep = _history_layer(env, policy, hist, T, N, noise_uniforms)
        elif noise_uniforms is not None:
            raise ValueError("noise_uniforms needs an env with an observation history")
        priv = abi.lg_runner_privileged(history=C.pointer(layer) if layer is not None else None, critic_normalizer=crit.handle if crit is not None else None,
                                        privileged_observations=out["privileged_observations"].data_ptr(), last_observations=last.data_ptr() if last is not None else None)
        call, name, tail = lib.lg_runner_collect_privileged, "lg_runner_collect_privileged", (C.byref(priv),)
    first = env.core.ctx
    if sensors is not None:          # the rig in the place of the context it is attached to
        call, name, first = lib.lg_runner_collect_sensors, "lg_runner_collect_sensors", sensors.handle
        sensors.begin()
    if not getattr(policy, "is_recurrent", False):
        rc = call(first, None, policy.actor.handle, None, policy.critic.handle, *head, None, None, None, None, None, C.byref(hooks), *tail, stream)
    else:
        mems, hidden, state, stacks = _hidden_rows(policy, T, N)
        rc = call(first, mems[0], policy.actor.handle, mems[1], policy.critic.handle, *head, C.byref(hidden), *state, C.byref(hooks), *tail, stream)
        out.update(stacks)
    _check(rc, name)
    del keep
    if sensors is not None:
        policy._call += T
        sensors.finish(T)
    else:
        _advance(env, policy, T)
    if last is not None:
        env.obs_buf = last
    out.update(extra)
    return out


def _history_layer(env, policy, hist, T, N, noise_uniforms):
    """`abi.lg_obs_history` over `env.obs_history` as `collect_distillation` and the privileged collector hand it to the library, and the tensors
    it points into (keep them alive until the call returns)."""
    dev = policy.device
    if not (hist.is_contiguous() and hist.dtype == torch.float32 and hist.shape[0] == N):
        raise ValueError("env.obs_history must be a contiguous float32 (N, H, W) tensor")
    H, W = hist.shape[1], hist.shape[2]
    scale = env.noise_scale_vec[:H * W].to(dev, torch.float32).contiguous() if getattr(env, "add_noise", False) else None
    if noise_uniforms is not None:
        noise_uniforms = noise_uniforms.to(dev, torch.float32).contiguous()
        assert noise_uniforms.shape == (T, N, H * W)
    layer = abi.lg_obs_history(history=hist.data_ptr(), H=H, W=W, noise_scale=scale.data_ptr() if scale is not None else None,
                               clip=float(env.cfg.normalization.clip_observations), noise_seed=(policy.seed ^ 0x5DEECE66D) & (2 ** 64 - 1),
                               inject_u=noise_uniforms.data_ptr() if noise_uniforms is not None else None)
    return layer, [scale, noise_uniforms]


def obs_history_step(history, obs, dones=None, noise_scale=None, clip=float("inf"), noise_uniforms=None, seed=0, call=0):
    """`lg_obs_history_step` (include/lgpolicy.h): one step of an observation-history layer, `student_history_update` + clip
    (`envs/anymal_c/anymal.py`) in one launch.  history (N, H, W) float32 contiguous, updated IN PLACE; obs (N, >= W): its first W columns enter
    slot 0 (rows may be strided); dones (N) or None; noise_scale (H W) or None: no noise; noise_uniforms (N, H W) replaces the Philox draws of
    (seed, call).  Returns the clipped observations (N, H W)."""
    lib = _lib()
    assert history.is_cuda and history.dtype == torch.float32 and history.is_contiguous() and history.dim() == 3
    N, H, W = history.shape
    dev = history.device
    obs = obs.to(dev, torch.float32)
    if obs.stride(1) != 1:
        obs = obs.contiguous()
    assert obs.shape[0] == N and obs.shape[1] >= W

    def opt(x, shape):
        if x is None:
            return None
        x = x.to(dev, torch.float32).contiguous()
        assert x.shape == shape, (tuple(x.shape), shape)
        return x
    dones, scale, u = opt(dones, (N,)), opt(noise_scale, (H * W,)), opt(noise_uniforms, (N, H * W))
    out = torch.empty(N, H * W, device=dev)
    _check(lib.lg_obs_history_step(_ptr(history), N, H, W, _ptr(obs), obs.stride(0), _ptr(dones), _ptr(scale), _ptr(u), int(seed), int(call), float(clip),
                                   _ptr(out), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lg_obs_history_step")
    return out


def collect_distillation(env, policy, num_steps, noise_uniforms=None):
    """The collection loop of `OnPolicyRunner.learn` with `Distillation.act` / `process_env_step` (`rsl_rl/algorithms/distillation.py:89-105`) as ONE call
    into the library (`lg_collect_distillation`, include/lgpolicy.h).  env: a native `LeggedRobot`; policy: `NativeStudentTeacher` or
    `NativeStudentTeacherRecurrent`.  Returns the (T, N, .) tensors `RolloutStorage` holds in "distillation" mode (`storage/rollout_storage.py:65-67,
    102-104`): observations, privileged_observations, actions, privileged_actions, rewards (the env's raw reward: no time-out bootstrap), dones.
    Draws the same samples as `num_steps` calls of `policy.act_and_teach`.

    An env with an observation history (`AnymalStudent`: `obs_history`, (N, H, 48)) hands that buffer to the library, which steps it in place
    (`lg_obs_history_step`); `env.obs_buf` is left as the student's observation after the last step, so a following `env.step` or
    `collect_distillation` continues the same history.  Noise follows `env.add_noise`, drawn by Philox (seed derived from the policy's, call = the
    sampling call); `noise_uniforms` (T, N, H * 48) replaces the draws (the checker mode).  Any other env: the student reads the first columns of
    the env's observation row.  Recurrent policy: also `hidden_states`, the `(memory_s, memory_t)` state BEFORE step 0 in `get_hidden_states()` form --
    distillation keeps no per-step hidden rows; this seeds `policy.reset(hidden_states=...)` of the update."""
    return _collect_distillation(env, policy, num_steps, noise_uniforms)


def _collect_distillation(env, policy, num_steps, noise_uniforms, hooks=None):
    """The body of `collect_distillation` (hooks None: `lg_collect_distillation*`) and of `collect_distillation_tracked` (an
    `abi.lg_runner_distill`: `lg_runner_collect_distillation*`, include/lgrunner_distill.h)."""
    lib = _lib()
    name = "lg_collect_distillation"
    if hooks is not None:
        from .normalizer import _runner_lib
        lib, name = _runner_lib(), "lg_runner_collect_distillation"
    dev = policy.device
    rec = getattr(policy, "is_recurrent", False)
    T, N, Ot, A = int(num_steps), env.core.t["obs_buf"].shape[0], env.core.t["obs_buf"].shape[1], policy.num_actions
    Os = policy.memory_s.input_size if rec else policy.student.dims[0]
    out = dict(observations=empty(dev, T, N, Os), privileged_observations=empty(dev, T, N, Ot), actions=empty(dev, T, N, A),
               privileged_actions=empty(dev, T, N, A), rewards=empty(dev, T, N, 1), dones=empty(dev, T, N, 1))
    last = empty(dev, N, Os)
    rows = abi.lg_distill_rollout(last_observations=last.data_ptr(), **{k: v.data_ptr() for k, v in out.items()})
    hist = getattr(env, "obs_history", None)
    layer, keep = None, []
    if hist is not None:
        layer, keep = _history_layer(env, policy, hist, T, N, noise_uniforms)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lp = C.byref(layer) if layer is not None else None
    tail = () if hooks is None else (C.byref(hooks),)
    if rec:
        mems = (policy.memory_s, policy.memory_t)
        before = []
        for m in mems:
            if m is not None:
                m.ensure_state(N)
            before.append(None if m is None else [torch.empty_like(m.h)] + ([torch.empty_like(m.c)] if m.rnn_type == "lstm" else []))
        p0 = [[_ptr(b) for b in bs] + [None] * (2 - len(bs)) if bs is not None else [None, None] for bs in before]
        live = [m._ptrs() if m is not None else (None, None) for m in mems]
        call = lib.lg_collect_distillation_recurrent if hooks is None else lib.lg_runner_collect_distillation_recurrent
        rc = call(env.core.ctx, mems[0].handle, policy.student.handle, mems[1].handle if mems[1] is not None else None,
                  policy.teacher.handle, _ptr(policy.std), policy.seed, policy._call + 1, T, lp, C.byref(rows),
                  *p0[0], *p0[1], *live[0], *live[1], *tail, stream)
        out["hidden_states"] = tuple(None if bs is None else (tuple(bs) if len(bs) == 2 else bs[0]) for bs in before)
    else:
        call = lib.lg_collect_distillation if hooks is None else lib.lg_runner_collect_distillation
        rc = call(env.core.ctx, policy.student.handle, policy.teacher.handle, _ptr(policy.std), policy.seed, policy._call + 1, T, lp,
                  C.byref(rows), *tail, stream)
    _check(rc, name)
    del keep
    _advance(env, policy, T)
    if hist is not None:
        env.obs_buf = last
    return out


def collect_distillation_tracked(env, policy, num_steps, obs_normalizer=None, privileged_obs_normalizer=None, episode_tracker=None, noise_uniforms=None):
    """`collect_distillation` through `lg_runner_collect_distillation` / `lg_runner_collect_distillation_recurrent` (include/lgrunner_distill.h),
    with the runner's device pieces between the launches of the one call.  Same dict; nothing given: the same rows, bit for bit.
    obs_normalizer (`NativeEmpiricalNormalization`, the student's width) and privileged_obs_normalizer (the teacher's, the env's row): every new
    row of a stream is normalised (and counted in training mode; one mode for both, `ValueError` otherwise) before it is stored and before the next
    act (`on_policy_runner.py:425-427`); row 0 is the normaliser's carried row -- the normalised row after the previous collection's last step --
    or, when it holds none, the raw one, as the first observations of `learn()` (`:364-366`).  A stream without a normaliser stays raw.
    `env.obs_buf` is left as the student's un-normalised row after the last step, and the env's privileged row stays raw.
    episode_tracker (`EpisodeTracker`): adds `raw_rewards` (T, N, 1) (equal to `rewards`: distillation stores the env's reward as it is),
    `episode_extras` (T, K), and `ep_return` / `ep_length` (T, N, 1), defined where `dones > 0`, as `collect_rollout_tracked` returns them; the
    tracker's live sums advance in place."""
    T, N = int(num_steps), env.core.t["obs_buf"].shape[0]
    hooks = abi.lg_runner_distill(student_normalizer=obs_normalizer.handle if obs_normalizer is not None else None,
                                  teacher_normalizer=privileged_obs_normalizer.handle if privileged_obs_normalizer is not None else None,
                                  training=_one_mode(obs_normalizer, privileged_obs_normalizer))
    extra = _episode_hook(hooks, env, episode_tracker, T, N, policy.device)
    out = _collect_distillation(env, policy, T, noise_uniforms, hooks)
    out.update(extra)
    return out


def estimation_row(env):
    """`TerrainEstimatorRunner._get_environment_data` (`rsl_rl/runners/terrain_estimator_runner.py:247-277`) on an env with both sensors: the
    camera's latest frame (a view of its FIFO), `cat[base_lin_vel, base_ang_vel]`, the ray caster's un-normalised distances."""
    depth = env.get_depth_images() if hasattr(env, "get_depth_images") else None
    if depth is None or not hasattr(env, "_get_raycast_distances"):
        raise ValueError("collect_estimation needs an env with the depth camera and the ray caster enabled (e.g. elspider_air_rough_raycast)")
    if depth.dim() == 4:
        depth = depth[:, -1]
    return depth, torch.cat([env.base_lin_vel, env.base_ang_vel], dim=-1), env._get_raycast_distances(normalize=False)


def collect_estimation(env, policy, num_steps, estimator=None, one_call=False, actions=None):
    """The data-collection loop of `TerrainEstimatorRunner.learn` (`rsl_rl/runners/terrain_estimator_runner.py:392-438`) over an env that carries
    the depth camera and the ray caster.  Per step t: the camera's latest frame, `cat[base_lin_vel, base_ang_vel]` and the un-normalised ray
    distances are copied into row t of preallocated (T, N, .) tensors (what `EstimatorRolloutStorage.add_transitions` keeps,
    `algorithms/distillation.py:398-407`), the env is stepped with `policy.act_inference(env.obs_buf)` (a native policy; `policy=None`:
    `0.5 * randn`, as `:427`), and `dones[t]` = the step's `reset_buf`.  The reference's storage never fills its `dones` (they stay zero, so its
    update never resets the memory at an episode boundary); the REAL ones are returned here.  A host loop over `env.step`: the sensors are driven
    from the env classes.  A policy with a `reset` method (a recurrent one: its memory) is reset on every step's dones, as the one call of
    `collect_estimation_driven` (`rl/estimator_runner.py`) resets it.

    Returns a dict: depth_images (T, N, h, w), proprio_data (T, N, 6), raycast_targets (T, N, R), dones (T, N).  With `estimator`
    (a `NativeTerrainEstimator`) it is also stepped on every row and reset on `dones[t]` after the step (`distillation.py:275`): the evaluation
    loop of `play` (`:637-730`), adding predictions (T, N, R) and the per-step `mse` / `mae` (T) it prints (`:666-670`).

    `actions` (T, N, A), with `policy=None`: the env is stepped with `actions[t]` instead of a draw.
    `one_call=True`: the same loop as ONE call into the library (`lg_collect_estimation`, include/lgsensors.h) on the env's `SensorRig`
    (`rl/sensors.py`; built on first use, `ValueError` where the rig refuses the env).  `policy` must be a native feed-forward policy exposing its
    actor (`policy.actor`, a `NativeMLP`: it reads the env's raw row, or its first columns when it is narrower), or None together with `actions`.
    The same dict, bit for bit, except `raycast_targets`' relation to `torch.norm`: the kernel takes torch's order of fp32 roundings, which holds
    as long as torch keeps it.  `mse` / `mae` are the two expressions above on the returned rows."""
    T = int(num_steps)
    if one_call:
        return _collect_estimation_one_call(env, policy, T, estimator, actions)
    if actions is not None and policy is not None:
        raise ValueError("collect_estimation: give a policy or actions, not both")
    depth, proprio, target = estimation_row(env)
    N, dev = depth.shape[0], depth.device
    out = dict(depth_images=torch.empty(T, N, *depth.shape[1:], device=dev), proprio_data=torch.empty(T, N, proprio.shape[1], device=dev),
               raycast_targets=torch.empty(T, N, target.shape[1], device=dev), dones=torch.empty(T, N, device=dev))
    if estimator is not None:
        out.update(predictions=torch.empty(T, N, target.shape[1], device=dev), mse=torch.empty(T, device=dev), mae=torch.empty(T, device=dev))
    for t in range(T):
        if t > 0:
            depth, proprio, target = estimation_row(env)
        out["depth_images"][t].copy_(depth)
        out["proprio_data"][t].copy_(proprio)
        out["raycast_targets"][t].copy_(target)
        if estimator is not None:
            pred = estimator.act_inference(depth, proprio)
            out["predictions"][t].copy_(pred)
            out["mse"][t] = torch.mean((pred - target) ** 2)
            out["mae"][t] = torch.mean(torch.abs(pred - target))
        if actions is not None:
            step_actions = actions[t]
        elif policy is None:
            step_actions = torch.randn(N, env.num_actions, device=env.device) * 0.5
        else:
            step_actions = policy.act_inference(env.obs_buf)
        dones = env.step(step_actions)[3]
        out["dones"][t].copy_(dones)
        if estimator is not None:
            estimator.reset(dones)
        if hasattr(policy, "reset"):          # a recurrent policy's memory (`Memory.reset(dones)`); nothing for a feed-forward one
            policy.reset(dones)
    return out


def _collect_estimation_one_call(env, policy, T, estimator, actions):
    """`collect_estimation(one_call=True)`: the checks the host can make, the rows, the one call, the rig's bookkeeping, `mse` / `mae`."""
    from .sensors import SensorRig, _sensor_lib
    if (policy is None) == (actions is None):
        raise ValueError("collect_estimation(one_call=True): exactly one of policy and actions must be given"
                         + (" (no policy: the actions come pre-drawn, (T, N, A))" if policy is None else ""))
    actor = None
    if policy is not None:
        actor = getattr(policy, "actor", None)
        if getattr(policy, "is_recurrent", False) or getattr(actor, "handle", None) is None or not hasattr(actor, "dims"):
            raise ValueError("collect_estimation(one_call=True): policy must be a native feed-forward policy exposing its actor (policy.actor, a NativeMLP)")
    rig = SensorRig.from_env(env, camera=True)
    if not (rig.has_rays and rig.has_camera):
        raise ValueError("collect_estimation(one_call=True): the env's rig must carry both the ray caster and the depth camera")
    lib = _sensor_lib()
    depth = env.get_depth_images()
    N, dev, R = depth.shape[0], depth.device, env.ray_caster.num_rays
    if actions is not None:
        actions = actions.to(dev, torch.float32).contiguous()
        if actions.shape != (T, N, env.num_actions):
            raise ValueError(f"actions of shape {tuple(actions.shape)}, expected {(T, N, env.num_actions)}")
    out = dict(depth_images=torch.empty(T, N, *depth.shape[2:], device=dev), proprio_data=torch.empty(T, N, 6, device=dev),
               raycast_targets=torch.empty(T, N, R, device=dev), dones=torch.empty(T, N, device=dev))
    nets = None
    if estimator is not None:
        out["predictions"] = torch.empty(T, N, estimator.num_raycast_outputs, device=dev)
        estimator.memory.ensure_state(N)
        h, c = estimator.memory._ptrs()
        nets = abi.lg_estimation_nets(encoder=estimator.encoder.handle, combine=estimator.combine.handle, memory=estimator.memory.handle,
                                      decoder=estimator.decoder.handle, h=h, c=c)
    rows = abi.lg_estimation_out(**{k: out[k].data_ptr() for k in ("depth_images", "proprio_data", "raycast_targets", "dones", "predictions") if k in out})
    rig.begin()
    _check(lib.lg_collect_estimation(rig.handle, actor.handle if actor is not None else None, _ptr(actions), T, C.byref(rows),
                                     C.byref(nets) if nets is not None else None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lg_collect_estimation")
    rig.finish(T)
    if estimator is not None:
        out.update(mse=torch.empty(T, device=dev), mae=torch.empty(T, device=dev))
        for t in range(T):
            pred, target = out["predictions"][t], out["raycast_targets"][t]
            out["mse"][t] = torch.mean((pred - target) ** 2)
            out["mae"][t] = torch.mean(torch.abs(pred - target))
    return out

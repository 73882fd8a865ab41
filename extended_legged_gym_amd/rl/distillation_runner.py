"""`NativeDistillationRunner`: the surface of rsl_rl's `OnPolicyRunner` (`runners/on_policy_runner.py`) for `training_type == "distillation"`
over the native pieces -- the one-call collection with two normalisers and the episode bookkeeping (`collect_distillation_tracked`,
include/lgrunner_distill.h) and the native updates (`NativeDistillation`, `NativeRecurrentDistillation`).  It needs neither `rsl_rl` nor
`tensorboard`; its checkpoints have rsl_rl's layout (`model_state_dict` in the order of `StudentTeacher(Recurrent).state_dict()`,
`optimizer_state_dict` as `torch.optim.Adam(policy.parameters()).state_dict()` holds it, `iter`, `infos`, and the two normaliser dicts).

The teacher comes from `runner.teacher_model_path` at construction (`:132-141`): the checkpoint the native (or rsl_rl's) PPO runner wrote for the
teacher task fills the teacher from `actor.*` and the teacher's normaliser from `obs_norm_state_dict`; a distillation checkpoint resumes
everything.  Refused by name: algorithms other than `Distillation`, policy classes other than `StudentTeacher` / `StudentTeacherRecurrent`,
`teacher_recurrent`, `multi_gpu_cfg`."""
import os
import statistics
import time

import torch

from .collector import EpisodeTracker, collect_distillation_tracked
from .normalizer import NativeEmpiricalNormalization
from .policy import TEACHER_MEMORY_MESSAGE
from .runner import ACTIVATIONS, RunnerLogging, _adam_group, _Memory, _mlp, _view_index, collects_privileged_natively, steps_outside_the_library

DISTILLATION_KEYS = ("num_learning_epochs", "gradient_length", "learning_rate", "max_grad_norm", "loss_type")
NO_TEACHER_PATH_MESSAGE = "Teacher model path not specified or does not exist. Please provide a valid path to the teacher model."
NO_TEACHER_MESSAGE = "Teacher model parameters not loaded. Please load a teacher model to distill."
NO_PARAMETERS_MESSAGE = "state_dict does not contain student or teacher parameters"


# ---------------------------------------------------------------------------------------------------------------- initial weights
class _StudentTeacher(torch.nn.Module):
    """The construction order and parameter names of `rsl_rl/modules/student_teacher.py:15-73` (student, teacher, `std`) and, with a memory in
    front of the student, of `modules/student_teacher_recurrent.py:15-69` (`memory_s` last).  Only its initial `state_dict()` is used."""

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims, teacher_hidden_dims, activation, init_noise_std, rnn=None):
        super().__init__()
        act = ACTIVATIONS[activation]
        self.student = _mlp([rnn["rnn_hidden_dim"] if rnn else num_student_obs] + list(student_hidden_dims) + [num_actions], act)
        self.teacher = _mlp([num_teacher_obs] + list(teacher_hidden_dims) + [num_actions], act)
        self.std = torch.nn.Parameter(init_noise_std * torch.ones(num_actions))
        if rnn:
            self.memory_s = _Memory(num_student_obs, rnn["rnn_type"], rnn["rnn_hidden_dim"], rnn["rnn_num_layers"])


def memory_settings(policy_cfg):
    """`rnn_type`, `rnn_hidden_dim`, `rnn_num_layers` of a `StudentTeacherRecurrent` config; the deprecated `rnn_hidden_size` counts where
    `rnn_hidden_dim` is at its default (`student_teacher_recurrent.py:33-40`)."""
    hidden = int(policy_cfg.get("rnn_hidden_dim", 256))
    if "rnn_hidden_size" in policy_cfg and hidden == 256:
        hidden = int(policy_cfg["rnn_hidden_size"])
    return dict(rnn_type=str(policy_cfg.get("rnn_type", "lstm")).lower(), rnn_hidden_dim=hidden, rnn_num_layers=int(policy_cfg.get("rnn_num_layers", 1)))


def initial_distillation_state_dict(policy_class_name, num_student_obs, num_teacher_obs, num_actions, policy_cfg, seed):
    """The `state_dict()` of a freshly initialised `StudentTeacher` / `StudentTeacherRecurrent` (torch's default initialisation, drawn under
    `seed` without disturbing the global generator), in the module's order: `std`, `student.N.*`, `teacher.N.*`, `memory_s.rnn.*`."""
    if policy_class_name not in ("StudentTeacher", "StudentTeacherRecurrent"):
        raise NotImplementedError(f"policy_class_name {policy_class_name}: the native distillation runner builds StudentTeacher and StudentTeacherRecurrent")
    if policy_cfg.get("teacher_recurrent", False):
        raise NotImplementedError(TEACHER_MEMORY_MESSAGE)
    activation = policy_cfg.get("activation", "elu")
    if activation not in ACTIVATIONS:
        raise ValueError(f"Unknown activation: {activation}")
    rnn = memory_settings(policy_cfg) if policy_class_name == "StudentTeacherRecurrent" else None
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        module = _StudentTeacher(int(num_student_obs), int(num_teacher_obs), int(num_actions), policy_cfg.get("student_hidden_dims", [256, 256, 256]),
                                 policy_cfg.get("teacher_hidden_dims", [256, 256, 256]), activation, float(policy_cfg.get("init_noise_std", 0.1)), rnn)
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------- checkpoint layout (no GPU)
def distillation_parameter_order(names):
    """The order of `policy.parameters()` (and of `state_dict()`) in the reference module, from any ordering of the names: the module's own
    parameter (`std`) first, then `student`, `teacher`, `memory_s`, `memory_t` in registration order, each in its own order."""
    names = list(names)
    rnn_order = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")

    def within(name):          # nn.Sequential: by layer index, weight before bias; nn.LSTM / nn.GRU: by layer, then torch's four tensors
        tail = name.split(".")[1:]
        if tail[0] == "rnn":
            kind, layer = tail[1].rsplit("_l", 1)
            return (int(layer), rnn_order.index(kind))
        return (int(tail[0]), ("weight", "bias").index(tail[1]))
    try:
        groups = [[n for n in names if n == "std"]] + [sorted((n for n in names if n.startswith(p + ".")), key=within)
                                                       for p in ("student", "teacher", "memory_s", "memory_t")]
    except (ValueError, IndexError) as e:
        raise KeyError(f"a name outside a StudentTeacher(Recurrent): {e}") from e
    ordered = [n for g in groups for n in g]
    if sorted(ordered) != sorted(names):
        raise KeyError(f"names outside a StudentTeacher(Recurrent): {sorted(set(names) - set(ordered))}")
    return ordered


def is_trained(name):
    """The tensors that ever receive a gradient in `Distillation.update` (`distillation.py:120-140`: the loss goes through `act_inference` alone)."""
    return name.startswith("student.") or name.startswith("memory_s.")


def distillation_adam_state_dict(optimizer_state, names):
    """A trainer's `optimizer_state()` (dicts `exp_avg`, `exp_avg_sq`, `parameters` over the trained names, `step`, `learning_rate`) and the names
    of the whole state dict -> what `torch.optim.Adam(policy.parameters(), lr).state_dict()` holds: one group over ALL parameters in
    `distillation_parameter_order`, and state entries (`step` a float32 scalar, `exp_avg`, `exp_avg_sq`) only for the trained ones, which are
    the only ones torch's lazy state initialisation ever reaches; an optimiser that has not stepped holds no state."""
    names = distillation_parameter_order(names)
    trained = [n for n in names if is_trained(n)]
    if sorted(trained) != sorted(optimizer_state["exp_avg"].keys()):
        raise KeyError(f"the optimiser's tensors {sorted(optimizer_state['exp_avg'].keys())} are not the trained ones {sorted(trained)}")
    state = {}
    if int(optimizer_state["step"]) > 0:
        for i, n in enumerate(names):
            if is_trained(n):
                state[i] = {"step": torch.tensor(float(optimizer_state["step"]), dtype=torch.float32),
                            "exp_avg": optimizer_state["exp_avg"][n].detach().cpu().clone(), "exp_avg_sq": optimizer_state["exp_avg_sq"][n].detach().cpu().clone()}
    return {"state": state, "param_groups": [_adam_group(optimizer_state["learning_rate"], len(names))]}


def native_distillation_optimizer_state(model_state_dict, adam):
    """The inverse: a checkpoint's `model_state_dict` and `optimizer_state_dict` -> the dict a trainer's `load_optimizer_state` takes."""
    names = distillation_parameter_order(model_state_dict.keys())
    group = adam["param_groups"][0]
    if len(adam["param_groups"]) != 1 or list(group["params"]) != list(range(len(names))):
        raise ValueError("optimizer_state_dict: expected one parameter group over the policy's parameters in order")
    state, steps = adam["state"], set()
    params, avg, sq = {}, {}, {}
    for i, n in enumerate(names):
        entry = state.get(i)
        if not is_trained(n):
            if entry is not None:
                raise ValueError(f"optimizer_state_dict: parameter {i} ({n}) holds moments, but distillation never trains it")
            continue
        params[n] = model_state_dict[n].detach().cpu()
        if entry is None:
            avg[n], sq[n] = torch.zeros_like(params[n]), torch.zeros_like(params[n])
            steps.add(0)
        else:
            avg[n], sq[n] = entry["exp_avg"].detach().cpu().to(torch.float32), entry["exp_avg_sq"].detach().cpu().to(torch.float32)
            steps.add(int(float(entry["step"])))
            if avg[n].shape != params[n].shape:
                raise ValueError(f"optimizer_state_dict: moment {i} has shape {tuple(avg[n].shape)}, parameter {n} {tuple(params[n].shape)}")
    if len(steps) != 1:
        raise ValueError(f"optimizer_state_dict: the parameters have different step counts {sorted(steps)}")
    return dict(parameters=params, exp_avg=avg, exp_avg_sq=sq, step=steps.pop(), learning_rate=float(group["lr"]))


def load_rule(keys, empirical_normalization):
    """What `OnPolicyRunner.load` (`:686-715`) does with a checkpoint whose `model_state_dict` has these keys, through
    `StudentTeacher.load_state_dict` (`student_teacher.py:111-146`).  Keys containing `actor`: a PPO checkpoint -- `actor.*` fills the teacher,
    nothing else of the model is read, the checkpoint's ACTOR normaliser is the teacher's and the student's is left alone, no optimiser, no
    iteration.  Else keys containing `student`: everything.  Else the reference's `ValueError`.  Returns a dict: `resumed`, `teacher_prefix`,
    `student` (the student, its memory and `std` are loaded), `normalizers` (runner attribute -> checkpoint key), `optimizer`, `iter`."""
    keys = list(keys)
    if any("actor" in k for k in keys):
        norms = {"privileged_obs_normalizer": "obs_norm_state_dict"} if empirical_normalization else {}
        return dict(resumed=False, teacher_prefix="actor", student=False, normalizers=norms, optimizer=False, iter=False)
    if any("student" in k for k in keys):
        norms = {"obs_normalizer": "obs_norm_state_dict", "privileged_obs_normalizer": "privileged_obs_norm_state_dict"} if empirical_normalization else {}
        return dict(resumed=True, teacher_prefix="teacher", student=True, normalizers=norms, optimizer=True, iter=True)
    raise ValueError(NO_PARAMETERS_MESSAGE)


def mlp_widths(state_dict, prefix):
    """[in, hidden..., out] of the `nn.Sequential` stored under `prefix.N.weight`."""
    idx = sorted(int(k[len(prefix) + 1:].split(".")[0]) for k in state_dict if k.startswith(prefix + ".") and k.endswith(".weight"))
    if not idx:
        return []
    return [int(state_dict[f"{prefix}.{idx[0]}.weight"].shape[1])] + [int(state_dict[f"{prefix}.{i}.weight"].shape[0]) for i in idx]


# ---------------------------------------------------------------------------------------------------------------- the runner
class NativeDistillationRunner(RunnerLogging):
    def __init__(self, env, train_cfg, log_dir=None, device="cuda:0"):
        from . import NativeDistillation, NativeRecurrentDistillation, NativeStudentTeacher, NativeStudentTeacherRecurrent
        self.cfg, self.alg_cfg, self.policy_cfg = dict(train_cfg["runner"]), dict(train_cfg["algorithm"]), dict(train_cfg["policy"])
        self.env, self.device, self.log_dir = env, torch.device(device), log_dir
        alg_name = self.alg_cfg.pop("class_name", self.cfg.get("algorithm_class_name", "Distillation"))
        if alg_name != "Distillation":
            raise NotImplementedError(f"algorithm_class_name {alg_name}: the native distillation runner runs Distillation (rl.NativeOnPolicyRunner runs PPO)")
        if self.alg_cfg.get("multi_gpu_cfg"):
            raise NotImplementedError("multi_gpu_cfg is not built in the native runner")
        policy_name = self.policy_cfg.pop("class_name", self.cfg.get("policy_class_name", "StudentTeacher"))
        num_obs, num_priv = int(env.num_obs), getattr(env, "num_privileged_obs", None)
        self.num_teacher_obs = int(num_priv) if num_priv is not None else num_obs
        self.seed = int(train_cfg.get("seed", 1))
        sd = initial_distillation_state_dict(policy_name, num_obs, self.num_teacher_obs, env.num_actions, self.policy_cfg, self.seed)
        activation = self.policy_cfg.get("activation", "elu")
        self.recurrent = policy_name == "StudentTeacherRecurrent"
        if self.recurrent:
            policy = NativeStudentTeacherRecurrent(sd, activation=activation, rnn_type=memory_settings(self.policy_cfg)["rnn_type"], teacher_recurrent=False,
                                                   device=str(self.device), seed=self.seed)
        else:
            policy = NativeStudentTeacher(sd, activation=activation, device=str(self.device), seed=self.seed)
        policy.loaded_teacher = False          # (the teacher holds its initial draws until a checkpoint fills it: student_teacher.py:36)
        kw = {k: self.alg_cfg[k] for k in DISTILLATION_KEYS if k in self.alg_cfg}
        self.alg = (NativeRecurrentDistillation if self.recurrent else NativeDistillation)(policy, sd, **kw)
        self.teacher_widths = mlp_widths(sd, "teacher")
        self.num_steps_per_env, self.save_interval = int(self.cfg["num_steps_per_env"]), int(self.cfg["save_interval"])
        self.empirical_normalization = bool(self.cfg.get("empirical_normalization", False))
        self.obs_normalizer = self.privileged_obs_normalizer = None
        if self.empirical_normalization:
            self.obs_normalizer = NativeEmpiricalNormalization([num_obs], until=int(1.0e8), device=str(self.device))
            self.privileged_obs_normalizer = NativeEmpiricalNormalization([self.num_teacher_obs], until=int(1.0e8), device=str(self.device))
        # an env the library can run whole collects through the one call; every other env through the host loop
        self.layered = not (collects_privileged_natively(env) or not steps_outside_the_library(env))
        self.writer, self.disable_logs = None, False
        self.tot_timesteps, self.tot_time, self.current_learning_iteration = 0, 0.0, 0
        self.resumed = False
        self._host_obs, self._host_priv, self._host_episode = None, None, None
        self.env.reset()
        teacher_model_path = self.cfg.get("teacher_model_path", None)          # on_policy_runner.py:132-141
        if teacher_model_path and os.path.exists(teacher_model_path):
            self.load(teacher_model_path)
            print(f"Loaded teacher model from {teacher_model_path}")
        else:
            raise ValueError(NO_TEACHER_PATH_MESSAGE)

    # ---- modes (`:729-754`: the teacher's normaliser follows the student's, in training mode too)
    def _normalizers(self):
        return [n for n in (self.obs_normalizer, self.privileged_obs_normalizer) if n is not None]

    def train_mode(self):
        for norm in self._normalizers():
            norm.train()

    def eval_mode(self):
        for norm in self._normalizers():
            norm.eval()

    def forget_carried(self):
        for norm in self._normalizers():
            norm.forget_carried()
        self._host_obs = self._host_priv = None

    # ---- collection
    def _collect(self, tracker):
        """One collection of `num_steps_per_env` steps: the dict of `collect_distillation_tracked`."""
        if not self.layered:
            return collect_distillation_tracked(self.env, self.alg.policy, self.num_steps_per_env, obs_normalizer=self.obs_normalizer,
                                                privileged_obs_normalizer=self.privileged_obs_normalizer, episode_tracker=tracker)
        return self._collect_host(tracker, self.num_steps_per_env)

    def _teacher_row(self, obs, priv=None):
        """`on_policy_runner.py:403-412`: the step's second value, else the getter, else the observations."""
        if priv is None:
            priv = self.env.get_privileged_observations() if hasattr(self.env, "get_privileged_observations") else None
        return (obs if priv is None else priv).to(self.device)

    def _collect_host(self, tracker, T):
        """The same dict from a host loop (`on_policy_runner.py:395-431` with `distillation.py:89-105`), for env classes whose step is more than
        the native one: `policy.act_and_teach`, `env.step`, the two normalisers, `policy.reset(dones)`."""
        env, policy, norm, pnorm, dev = self.env, self.alg.policy, self.obs_normalizer, self.privileged_obs_normalizer, self.device
        obs = self._host_obs if self._host_obs is not None else env.get_observations().to(dev)          # (the first rows pass no normaliser: :364-366)
        priv = self._host_priv if self._host_priv is not None else self._teacher_row(obs)
        N, A = env.num_envs, env.num_actions
        ex = env.core.t["extras_episode"]

        def z(*shape):
            return torch.empty(*shape, device=dev, dtype=torch.float32)
        d = dict(observations=z(T, N, obs.shape[1]), privileged_observations=z(T, N, priv.shape[1]), actions=z(T, N, A), privileged_actions=z(T, N, A),
                 rewards=z(T, N, 1), dones=z(T, N, 1))
        if policy.is_recurrent:
            policy.memory_s.ensure_state(N)
            hs = policy.memory_s.hidden_states
            d["hidden_states"] = (tuple(h.clone() for h in hs) if isinstance(hs, tuple) else hs.clone(), None)
        d.update(raw_rewards=z(T, N, 1), episode_extras=z(T, ex.numel()))
        self._host_episode = []
        for t in range(T):
            actions, teach = policy.act_and_teach(obs, priv)
            d["observations"][t], d["privileged_observations"][t], d["actions"][t], d["privileged_actions"][t] = obs, priv, actions, teach
            obs, priv, rew, dones, infos = env.step(actions)
            obs = obs.to(dev)
            priv = self._teacher_row(obs, priv)
            if norm is not None and pnorm is not None:
                obs, priv = norm.step_pair(pnorm, obs, priv)
            else:
                obs = norm(obs) if norm is not None else obs
                priv = pnorm(priv) if pnorm is not None else priv.clone()          # (the env's own buffer: the next step overwrites it)
            d["rewards"][t, :, 0] = d["raw_rewards"][t, :, 0] = rew          # Distillation.process_env_step: the env's reward as it is
            d["dones"][t, :, 0] = (dones != 0).float()
            d["episode_extras"][t] = ex
            self._host_episode.append({k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in infos.get("episode", {}).items()
                                       if not _view_index(v, ex)[0]})
            policy.reset(dones)
        self._host_obs, self._host_priv = obs.clone(), priv.clone()
        ep_return, ep_length = tracker.track(d["raw_rewards"], d["dones"])
        d["ep_return"], d["ep_length"] = ep_return.reshape(T, N, 1), ep_length.reshape(T, N, 1)
        return d

    # ---- the loop (`:347-486`)
    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        env = self.env
        if not self.alg.policy.loaded_teacher:          # :353-355
            raise ValueError(NO_TEACHER_MESSAGE)
        self._open_writer()
        if init_at_random_ep_len:
            env.episode_length_buf[:] = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
        self.forget_carried()
        self.train_mode()
        tracker = EpisodeTracker(env.num_envs, self.device)
        start_iter = self.current_learning_iteration
        tot_iter = start_iter + int(num_learning_iterations)
        for it in range(start_iter, tot_iter):
            start = time.time()
            rollout = self._collect(tracker)
            tracker.extend(rollout["dones"], rollout["ep_return"], rollout["ep_length"])          # (the one device-to-host copy of the collection)
            stop = time.time()
            collection_time, start = stop - start, stop
            loss_dict = self.alg.update(rollout)
            stop = time.time()
            learn_time = stop - start
            self.current_learning_iteration = it
            if self.log_dir is not None and not self.disable_logs:
                self.log(dict(it=it, tot_iter=tot_iter, start_iter=start_iter, num_learning_iterations=int(num_learning_iterations), collection_time=collection_time,
                              learn_time=learn_time, loss_dict=loss_dict, rewbuffer=tracker.rewbuffer, lenbuffer=tracker.lenbuffer,
                              episode=self._episode_means(rollout)))
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
            if self.cfg.get("multi_stage_rewards", False) and len(tracker.rewbuffer) > 0 and env.update_reward_scales(statistics.mean(tracker.rewbuffer)):
                print("Updated reward scales to ", env.reward_scales_stage)
                tracker.rewbuffer.clear()
                tracker.cur_reward_sum.zero_()
        if self.log_dir is not None and not self.disable_logs:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
            if hasattr(self.writer, "flush"):
                self.writer.flush()

    # ---- checkpoints (`:662-715`)
    def model_state_dict(self):
        sd = self.alg.state_dict()
        return {n: sd[n] for n in distillation_parameter_order(sd.keys())}

    def save(self, path, infos=None):
        model = self.model_state_dict()
        saved = {"model_state_dict": model, "optimizer_state_dict": distillation_adam_state_dict(self.alg.optimizer_state(), model.keys()),
                 "iter": self.current_learning_iteration, "infos": infos}
        if self.empirical_normalization:
            saved["obs_norm_state_dict"] = self.obs_normalizer.state_dict()
            saved["privileged_obs_norm_state_dict"] = self.privileged_obs_normalizer.state_dict()
        torch.save(saved, path)

    def load(self, path, load_optimizer=True):
        loaded = torch.load(path, map_location="cpu", weights_only=False)
        model = loaded["model_state_dict"]
        rule = load_rule(model.keys(), self.empirical_normalization)
        got = mlp_widths(model, rule["teacher_prefix"])
        if got != self.teacher_widths:
            raise ValueError(f"the checkpoint's {rule['teacher_prefix']} has layer widths {got}, but teacher_hidden_dims and the env give the teacher "
                             f"{self.teacher_widths}")
        if rule["student"]:
            want = distillation_parameter_order(self.alg.state_dict().keys())
            if sorted(model.keys()) != sorted(want):
                raise KeyError(f"model_state_dict does not hold this policy's parameters: missing {sorted(set(want) - set(model))}, "
                               f"unexpected {sorted(set(model) - set(want))}")
        for attr, key in rule["normalizers"].items():
            norm, state = getattr(self, attr), loaded[key]
            if state["_mean"].numel() != norm.num_features:
                raise ValueError(f"{key} holds {state['_mean'].numel()} columns, this runner's {attr} {norm.num_features}")
        self.alg.load_teacher(model)
        if rule["student"]:
            policy = self.alg.policy
            policy.std.copy_(model["std"].to(policy.std.device, torch.float32))
            self.alg.set_untrained("std", model["std"])
            if load_optimizer and rule["optimizer"] and "optimizer_state_dict" in loaded:
                self.alg.load_optimizer_state(native_distillation_optimizer_state(model, loaded["optimizer_state_dict"]))
            else:
                self.alg.load_state_dict(model)
        for attr, key in rule["normalizers"].items():
            getattr(self, attr).load_state_dict(loaded[key])
        self.forget_carried()
        if rule["iter"]:
            self.current_learning_iteration = loaded["iter"]
        self.resumed = self.alg.policy.resumed = rule["resumed"]
        return loaded.get("infos")

    def get_inference_policy(self, device=None):
        self.eval_mode()
        policy = self.alg.policy.act_inference
        if self.empirical_normalization:
            norm = self.obs_normalizer
            return lambda x: policy(norm(x))
        return policy

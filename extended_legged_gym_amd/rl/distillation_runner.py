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

import torch

from .collector import collect_distillation_tracked, empty
from .policy import TEACHER_MEMORY_MESSAGE
from .runner import (ACTIVATIONS, NativeRunner, _clone_state, _Memory, _mlp, checked_activation, collects_privileged_natively, from_adam_state_dict,
                     seeded_state_dict, steps_outside_the_library, to_adam_state_dict)

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
    activation = checked_activation(policy_cfg)
    rnn = memory_settings(policy_cfg) if policy_class_name == "StudentTeacherRecurrent" else None
    return seeded_state_dict(seed, _StudentTeacher, int(num_student_obs), int(num_teacher_obs), int(num_actions), policy_cfg.get("student_hidden_dims", [256, 256, 256]),
                             policy_cfg.get("teacher_hidden_dims", [256, 256, 256]), activation, float(policy_cfg.get("init_noise_std", 0.1)), rnn)


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
    """A distillation trainer's `optimizer_state()` and the names of the whole state dict -> `torch.optim.Adam(policy.parameters(), lr).state_dict()`:
    one group over ALL parameters in `distillation_parameter_order`, state entries only for the `is_trained` ones (`runner.to_adam_state_dict`)."""
    return to_adam_state_dict(optimizer_state, names, distillation_parameter_order, is_trained)


def native_distillation_optimizer_state(model_state_dict, adam):
    """The inverse: a checkpoint's `model_state_dict` and `optimizer_state_dict` -> the dict a trainer's `load_optimizer_state` takes."""
    return from_adam_state_dict(model_state_dict, adam, distillation_parameter_order, is_trained)


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
class NativeDistillationRunner(NativeRunner):
    _parameter_order = staticmethod(distillation_parameter_order)          # `StudentTeacher(Recurrent).parameters()`, and its `state_dict()`

    def __init__(self, env, train_cfg, log_dir=None, device="cuda:0"):
        from . import NativeDistillation, NativeRecurrentDistillation, NativeStudentTeacher, NativeStudentTeacherRecurrent
        alg_name, policy_name = self._configure(env, train_cfg, log_dir, device, "Distillation", "StudentTeacher")
        if alg_name != "Distillation":
            raise NotImplementedError(f"algorithm_class_name {alg_name}: the native distillation runner runs Distillation (rl.NativeOnPolicyRunner runs PPO)")
        if self.alg_cfg.get("multi_gpu_cfg"):
            raise NotImplementedError("multi_gpu_cfg is not built in the native runner")
        num_obs, num_priv = int(env.num_obs), getattr(env, "num_privileged_obs", None)
        self.num_teacher_obs = int(num_priv) if num_priv is not None else num_obs
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
        self.resumed = False
        # an env the library can run whole collects through the one call; every other env through the host loop
        self._start([num_obs, self.num_teacher_obs], layered=not (collects_privileged_natively(env) or not steps_outside_the_library(env)))
        teacher_model_path = self.cfg.get("teacher_model_path", None)          # on_policy_runner.py:132-141
        if teacher_model_path and os.path.exists(teacher_model_path):
            self.load(teacher_model_path)
            print(f"Loaded teacher model from {teacher_model_path}")
        else:
            raise ValueError(NO_TEACHER_PATH_MESSAGE)

    def _normalizers(self):
        """The student's handle and the teacher's, which follows the student's mode, in training too (`:736-738`)."""
        return self.obs_normalizer, self.privileged_obs_normalizer

    def _before_learn(self):          # :353-355
        if not self.alg.policy.loaded_teacher:
            raise ValueError(NO_TEACHER_MESSAGE)

    # ---- collection: `Distillation.act` / `process_env_step` (`distillation.py:89-105`)
    def _collect_one_call(self, tracker):
        return collect_distillation_tracked(self.env, self.alg.policy, self.num_steps_per_env, obs_normalizer=self.obs_normalizer,
                                            privileged_obs_normalizer=self.privileged_obs_normalizer, episode_tracker=tracker)

    def _host_rows(self, T, N, obs, priv):
        A, dev, policy = self.env.num_actions, self.device, self.alg.policy
        d = dict(observations=empty(dev, T, N, obs.shape[1]), privileged_observations=empty(dev, T, N, priv.shape[1]), actions=empty(dev, T, N, A),
                 privileged_actions=empty(dev, T, N, A), rewards=empty(dev, T, N, 1), dones=empty(dev, T, N, 1))
        if policy.is_recurrent:          # the `(memory_s, memory_t)` state BEFORE step 0: distillation keeps no per-step hidden rows
            policy.memory_s.ensure_state(N)
            d["hidden_states"] = (_clone_state(policy.memory_s.hidden_states), None)
        return d

    def _host_act(self, d, t, obs, priv):          # `Distillation.act` (`distillation.py:89-96`)
        actions, teach = self.alg.policy.act_and_teach(obs, priv)
        d["actions"][t], d["privileged_actions"][t] = actions, teach
        return actions

    def _host_reward(self, d, t, rew, infos):          # `Distillation.process_env_step` (`distillation.py:98-105`): the env's reward as it is
        d["rewards"][t, :, 0] = rew

    # ---- checkpoints (`:662-715`)
    def _adam_state_dict(self, model):
        return distillation_adam_state_dict(self.alg.optimizer_state(), model.keys())

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

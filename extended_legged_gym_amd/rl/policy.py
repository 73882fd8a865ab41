"""`NativeActorCritic`: the feed-forward `ActorCritic` of the vendored rsl_rl (`modules/actor_critic.py:16-136`) with its two
MLPs evaluated by `lg_mlp_forward` / `lg_policy_act` (include/lgpolicy.h): all layers of a network in one launch on the fp32
matrix cores, and `PPO.act` (`algorithms/ppo.py:147-159`: sample, value, log-prob, mean, sigma) as ONE launch instead of
~25.  Inference only: the weights come from a trained / initialised torch `ActorCritic` (its `state_dict`); the gradients
are `rl.NativePPO`'s (`rl.NativeRecurrentPPO`'s for the recurrent policy below), which moves these weights in place.

`NativeActorCriticRecurrent`: rsl_rl's `ActorCriticRecurrent` (`modules/actor_critic_recurrent.py:16-85`: an `nn.LSTM` / `nn.GRU`
`Memory`, `networks/memory.py:16-51`, in front of each MLP) on `lg_rnn_step` / `lg_policy_act_recurrent`: one launch per memory layer
(both memories side by side) plus the `PPO.act` launch.  The hidden state lives in torch tensors the kernels update in place."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from extended_legged_gym_amd.native import load_library


def _lib():
    return load_library("policy", "policy_wide")


LOG_SQRT_2PI = 0.9189385332046727          # log sqrt(2 pi) of Normal.log_prob and Normal.entropy


def _ptr(x):
    """The device pointer of a tensor; NULL for None."""
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _error(name):
    """The library keeps one message per thread, whichever entry point failed (include/lgpolicy.h: `lg_mlp_last_error`)."""
    return RuntimeError(f"{name} failed: " + (_lib().lg_mlp_last_error(None) or b"").decode())


def _check(rc, name):
    if rc != abi.LG_OK:
        raise _error(name)


class _NativeHandle:
    """What the owners of a library handle share (`NativeMLP`, `NativeMemory`, `NativeConvEncoder`): the GPU check, `lib`, the device index, the
    current stream, `_check`, and `close` / `__del__` through the class's destroy function."""
    _destroy = None          # the name of the handle's destroy function
    _check = staticmethod(_check)

    def _open(self, device, kernels="policy"):
        """Sets `lib` and `device`; returns the device index the create function takes."""
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"the {kernels} kernels run on the GPU only (no CPU path)")
        self.lib, self.device = _lib(), dev
        return dev.index if dev.index is not None else torch.cuda.current_device()

    def _created(self, handle, name):
        if not handle:
            raise _error(name)
        self.handle = handle

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeMLP(_NativeHandle):
    """nn.Sequential(Linear, act, ..., Linear) on the GPU.  `layers`: list of (weight (out, in), bias (out))."""
    _destroy = "lg_mlp_destroy"

    def __init__(self, layers, activation="elu", device="cuda:0"):
        index = self._open(device)
        ws = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w, _ in layers]
        bs = [np.ascontiguousarray(np.asarray(b, dtype=np.float32)) for _, b in layers]
        dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        for i, w in enumerate(ws):
            assert w.shape == (dims[i + 1], dims[i]) and bs[i].shape == (dims[i + 1],)
        L = len(ws)
        fp = C.POINTER(C.c_float)
        wp = (fp * L)(*[w.ctypes.data_as(fp) for w in ws])
        bp = (fp * L)(*[b.ctypes.data_as(fp) for b in bs])
        self.dims = dims
        # an input row wider than one activation image (an observation that carries a sensor) takes the entry point with the split-K first layer
        create = "lg_mlp_create_wide" if dims[0] > abi.MLP_MAX_WIDTH else "lg_mlp_create"
        self._created(getattr(self.lib, create)(L, (C.c_int32 * (L + 1))(*dims), wp, bp, abi.ACTIVATIONS[activation], index), create)

    @classmethod
    def from_sequential_state(cls, state, prefix, activation="elu", device="cuda:0"):
        """Layers `prefix.0.weight`, `prefix.2.weight`, ... of an nn.Sequential state dict."""
        idx = sorted({int(k[len(prefix) + 1:].split(".")[0]) for k in state if k.startswith(prefix + ".") and k.endswith(".weight")})
        layers = [(state[f"{prefix}.{i}.weight"].detach().cpu().numpy(), state[f"{prefix}.{i}.bias"].detach().cpu().numpy()) for i in idx]
        return cls(layers, activation, device)

    def __call__(self, x):
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        assert x.dim() == 2 and x.shape[1] == self.dims[0]
        y = torch.empty(x.shape[0], self.dims[-1], device=self.device)
        self._check(self.lib.lg_mlp_forward(self.handle, _ptr(x), x.shape[0], _ptr(y), self._stream()), "lg_mlp_forward")
        return y


class _GaussianPolicy:
    """What `NativeActorCritic` and `NativeStudentTeacher` share: the `std` vector, the rows every act writes (`_actions`, `_mean`) with the Philox call
    number, and `action_mean` / `action_std` / `entropy` over them."""

    def _load_std(self, state_dict, noise_std_type="scalar"):
        if noise_std_type == "scalar":
            self.std = state_dict["std"].detach().to(self.device, torch.float32).contiguous()
        elif noise_std_type == "log":
            self.std = torch.exp(state_dict["log_std"].detach().to(self.device, torch.float32)).contiguous()
        else:
            raise ValueError(f"Unknown standard deviation type: {noise_std_type}. Should be 'scalar' or 'log'")

    def _f32(self, x):
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _rows(self, n):
        """Fresh output rows for one act on n rows, and the next call number."""
        self._actions = torch.empty(n, self.num_actions, device=self.device)
        self._mean = torch.empty(n, self.num_actions, device=self.device)
        self._call += 1

    @property
    def action_mean(self):
        return self._mean

    @property
    def action_std(self):
        return self.std.expand_as(self._mean)

    @property
    def entropy(self):
        return (0.5 + LOG_SQRT_2PI + torch.log(self.std)).sum().expand(self._mean.shape[0])


class NativeActorCritic(_GaussianPolicy):
    """Same surface as `ActorCritic` for rollout collection: `act`, `act_inference`, `evaluate`, `get_actions_log_prob`,
    `action_mean`, `action_std`, `entropy` (`actor_critic.py:96-136`)."""
    is_recurrent = False

    def __init__(self, state_dict, activation="elu", noise_std_type="scalar", device="cuda:0", seed=0):
        self.device = torch.device(device)
        self.actor = NativeMLP.from_sequential_state(state_dict, "actor", activation, device)
        self.critic = NativeMLP.from_sequential_state(state_dict, "critic", activation, device)
        self.noise_std_type = noise_std_type
        self._load_std(state_dict, noise_std_type)
        self.num_actions = self.actor.dims[-1]
        self.seed, self._call = int(seed), 0
        self._mean = self._actions = self._logp = self._values = None

    def reset(self, dones=None):
        pass

    def _rows(self, n, keep_values=True):
        """Returns the row the critic writes: `_values`, or a scratch row for an act whose critic output means nothing (`_values` stays)."""
        super()._rows(n)
        self._logp = torch.empty(n, device=self.device)
        values = torch.empty(n, self.critic.dims[-1], device=self.device)
        if keep_values:
            self._values = values
        return values

    def _act(self, obs, critic_obs, deterministic, keep_values=True):
        """`lg_policy_act` on prepared rows (a feed-forward policy's observations, a recurrent one's memory outputs)."""
        n = obs.shape[0]
        values = self._rows(n, keep_values)
        _check(self.actor.lib.lg_policy_act(self.actor.handle, self.critic.handle, _ptr(obs), _ptr(critic_obs), n, _ptr(self.std), self.seed, self._call,
                                            int(deterministic), _ptr(self._actions), _ptr(self._mean), _ptr(self._logp), _ptr(values),
                                            self.actor._stream()), "lg_policy_act")

    def _run(self, obs, critic_obs, deterministic):
        obs = self._f32(obs)
        self._act(obs, obs if critic_obs is None else self._f32(critic_obs), deterministic)

    def act_and_evaluate(self, obs, critic_obs=None):
        """`PPO.act` in one launch: (actions, values, actions_log_prob, action_mean, action_sigma)."""
        self._run(obs, critic_obs, False)
        return self._actions, self._values, self._logp, self._mean, self.action_std

    def act(self, observations, **kwargs):
        self._run(observations, None, False)
        return self._actions

    def act_inference(self, observations):
        return self.actor(observations)

    def evaluate(self, critic_observations, **kwargs):
        return self.critic(critic_observations)

    def get_actions_log_prob(self, actions):
        if actions is self._actions:
            return self._logp
        sd = self.std
        return (-((actions - self._mean) ** 2) / (2 * sd * sd) - torch.log(sd) - LOG_SQRT_2PI).sum(dim=-1)


class NativeMemory(_NativeHandle):
    """One `Memory` (`networks/memory.py:16-51`) in inference mode.  `layers`: per RNN layer (weight_ih, weight_hh, bias_ih, bias_hh) in torch's
    layout; input width, hidden width and depth come from the shapes.  The state (`h`, and `c` for an LSTM; (L, n, H)) is allocated, zeroed,
    on the first step and again when the number of rows changes, as `Memory` does with `hidden_states = None`."""
    _destroy = "lg_rnn_destroy"

    def __init__(self, layers, rnn_type="lstm", device="cuda:0"):
        index = self._open(device)
        rnn_type = rnn_type.lower()
        if rnn_type not in abi.RNN_TYPES:
            raise ValueError(f"Unknown rnn_type: {rnn_type}. Should be 'lstm' or 'gru'")
        self.rnn_type = rnn_type
        G = 4 if rnn_type == "lstm" else 3
        arrs = [[np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in layer] for layer in layers]
        self.num_layers, self.hidden_size, self.input_size = len(arrs), arrs[0][1].shape[1], arrs[0][0].shape[1]
        H = self.hidden_size
        for l, (wi, wh, bi, bh) in enumerate(arrs):
            assert wi.shape == (G * H, self.input_size if l == 0 else H) and wh.shape == (G * H, H) and bi.shape == bh.shape == (G * H,), \
                f"layer {l}: shapes do not belong to an nn.{rnn_type.upper()} of hidden size {H}"
        fp = C.POINTER(C.c_float)
        lists = [(fp * len(arrs))(*[layer[j].ctypes.data_as(fp) for layer in arrs]) for j in range(4)]
        # an input row wider than the one-launch layer holds (an observation that carries a sensor) takes the entry point with the projection in front
        create = "lg_rnn_create_wide" if self.input_size > abi.RNN_MAX_WIDTH else "lg_rnn_create"
        self._created(getattr(self.lib, create)(abi.RNN_TYPES[rnn_type], self.num_layers, self.input_size, H, *lists, index), create)
        self.h = self.c = None

    @classmethod
    def from_state(cls, state, prefix, rnn_type="lstm", device="cuda:0"):
        """Layers `prefix.rnn.weight_ih_l0`, ... of an `ActorCriticRecurrent` state dict."""
        L = len([k for k in state if k.startswith(prefix + ".rnn.weight_ih_l")])
        if L == 0:
            raise KeyError(f"no {prefix}.rnn.weight_ih_l0 in the state dict: not an ActorCriticRecurrent checkpoint")
        layers = [[state[f"{prefix}.rnn.{name}_l{l}"].detach().cpu().numpy() for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for l in range(L)]
        return cls(layers, rnn_type, device)

    def ensure_state(self, n):
        if self.h is None or self.h.shape[1] != n:
            self.h = torch.zeros(self.num_layers, n, self.hidden_size, device=self.device)
            self.c = torch.zeros_like(self.h) if self.rnn_type == "lstm" else None

    def set_state(self, hidden_states):
        """Installs `(h, c)` (LSTM) or `h` (GRU), each (L, n, H), as the live state, as `Memory.reset(hidden_states=...)` does; the tensors are
        copied.  None forgets the state."""
        if hidden_states is None:
            self.h = self.c = None
            return
        parts = hidden_states if isinstance(hidden_states, (tuple, list)) else (hidden_states,)
        self.h = parts[0].detach().to(self.device, torch.float32).clone().contiguous()
        self.c = parts[1].detach().to(self.device, torch.float32).clone().contiguous() if self.rnn_type == "lstm" else None

    def _ptrs(self):
        return _ptr(self.h), _ptr(self.c)

    @property
    def hidden_states(self):
        """As `Memory.hidden_states`: `(h, c)` for an LSTM, `h` for a GRU, None before the first step; views of the live state."""
        if self.h is None:
            return None
        return (self.h, self.c) if self.rnn_type == "lstm" else self.h

    def __call__(self, x, reset=None):
        """`Memory.forward(input)` (inference mode): advances the state, returns the top layer's h' (n, H) -- a view of the state."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        assert x.dim() == 2 and x.shape[1] == self.input_size
        n = x.shape[0]
        self.ensure_state(n)
        if reset is not None:
            reset = reset.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
        self._check(self.lib.lg_rnn_step(self.handle, _ptr(x), n, *self._ptrs(), _ptr(reset), None, self._stream()), "lg_rnn_step")
        return self.h[-1]

    def reset(self, dones=None):
        """`Memory.reset(dones)` (`memory.py:35-51`): None forgets the state; else rows with dones != 0 are zeroed."""
        if dones is None:
            self.h = self.c = None
        elif self.h is not None:
            d = dones.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
            assert d.shape[0] == self.h.shape[1]
            self._check(self.lib.lg_rnn_reset_rows(self.handle, *self._ptrs(), _ptr(d), d.shape[0], self._stream()), "lg_rnn_reset_rows")


class NativeActorCriticRecurrent(NativeActorCritic):
    """Same surface as `ActorCriticRecurrent` for rollout collection (`actor_critic_recurrent.py:62-85`): `act`, `act_inference`, `evaluate`,
    `reset(dones)`, `get_hidden_states`, and what `NativeActorCritic` has.  Built from an `ActorCriticRecurrent.state_dict()`
    (`memory_a.rnn.*`, `memory_c.rnn.*`, `actor.*`, `critic.*`, `std` / `log_std`).  The batch mode of `PPO.update` is not a method of this
    object (`masks=` / `hidden_states=` raise): `rl.NativeRecurrentPPO` runs it on the rollout dict and moves this object's weights in place."""
    is_recurrent = True

    def __init__(self, state_dict, activation="elu", rnn_type="lstm", noise_std_type="scalar", device="cuda:0", seed=0):
        super().__init__(state_dict, activation, noise_std_type, device, seed)
        self.memory_a = NativeMemory.from_state(state_dict, "memory_a", rnn_type, device)
        self.memory_c = NativeMemory.from_state(state_dict, "memory_c", rnn_type, device)
        if self.actor.dims[0] != self.memory_a.hidden_size or self.critic.dims[0] != self.memory_c.hidden_size:
            raise ValueError("the MLPs of an ActorCriticRecurrent take their memory's hidden state as input")

    @staticmethod
    def _no_batch_mode(masks, hidden_states):
        if masks is not None or hidden_states is not None:
            raise NotImplementedError("masks= / hidden_states= (the batch mode of PPO.update) is not a method of the native policy: rl.NativeRecurrentPPO runs "
                                      "the update on the rollout dict")

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def _run(self, obs, critic_obs, deterministic):
        obs = self._f32(obs)
        cobs = obs if critic_obs is None else self._f32(critic_obs)
        n = obs.shape[0]
        assert obs.shape[1] == self.memory_a.input_size and cobs.shape == (n, self.memory_c.input_size)
        self.memory_a.ensure_state(n)
        self.memory_c.ensure_state(n)
        self._rows(n)
        _check(self.actor.lib.lg_policy_act_recurrent(self.memory_a.handle, self.actor.handle, self.memory_c.handle, self.critic.handle, _ptr(obs), _ptr(cobs), n,
                                                      _ptr(self.std), self.seed, self._call, int(deterministic), *self.memory_a._ptrs(), *self.memory_c._ptrs(),
                                                      None, _ptr(self._actions), _ptr(self._mean), _ptr(self._logp), _ptr(self._values), self.actor._stream()),
               "lg_policy_act_recurrent")

    def act(self, observations, masks=None, hidden_states=None):
        """`ActorCriticRecurrent.act`: advances the ACTOR memory only (the critic's waits for `evaluate`); samples with `lg_policy_act` on its
        output, so the draw for (seed, call, row) is the one `act_and_evaluate` makes.  The critic MLP of that launch runs on zeros, unused."""
        self._no_batch_mode(masks, hidden_states)
        top = self.memory_a(observations)
        self._act(top, torch.zeros(top.shape[0], self.critic.dims[0], device=self.device), False, keep_values=False)
        return self._actions

    def act_inference(self, observations):
        return self.actor(self.memory_a(observations))

    def evaluate(self, critic_observations, masks=None, hidden_states=None):
        self._no_batch_mode(masks, hidden_states)
        return self.critic(self.memory_c(critic_observations))


TEACHER_MEMORY_MESSAGE = "Loading recurrent memory for the teacher is not implemented yet"


def _split_distillation_state(state_dict, student_state_dict):
    """The two loading rules of `StudentTeacher.load_state_dict` (`student_teacher.py:111-146`): a PPO checkpoint (`actor.*`) fills the teacher only --
    the student then comes from `student_state_dict` (`student.*`, `std`, `memory_s.*`) --, a distillation checkpoint (`student.*` / `teacher.*` / `std`)
    fills both.  Returns (dict with the teacher, dict with the student, teacher prefix, resumed)."""
    if any("actor" in k for k in state_dict):
        if student_state_dict is None or not any(k.startswith("student.") for k in student_state_dict):
            raise ValueError("a PPO checkpoint (actor.*) holds the teacher only: pass the student's parameters (student.*, std) as student_state_dict")
        return state_dict, student_state_dict, "actor", False
    if any("student" in k for k in state_dict):
        return state_dict, state_dict, "teacher", True
    raise ValueError("state_dict does not contain student or teacher parameters")


class NativeStudentTeacher(_GaussianPolicy):
    """Same surface as rsl_rl's `StudentTeacher` (`modules/student_teacher.py:75-152`) for collection with `Distillation` (`distillation.py:89-105`)
    and for `get_inference_policy`: `act`, `act_inference`, `evaluate`, `reset`, `get_hidden_states`, `action_mean`, `action_std`, `loaded_teacher`;
    `act_and_teach(obs, teacher_obs)` is `Distillation.act` as ONE launch (`lg_distill_act`).  Inference only: `Distillation.update` trains a torch
    `StudentTeacher` whose state dict builds this object, or `rl.NativeDistillation` moves this object's student in place."""
    is_recurrent = False

    def __init__(self, state_dict, student_state_dict=None, activation="elu", device="cuda:0", seed=0):
        self.device = torch.device(device)
        tsd, ssd, tprefix, self.resumed = _split_distillation_state(state_dict, student_state_dict)
        self._check_teacher_memory(tprefix)
        self._activation = activation
        self.teacher = NativeMLP.from_sequential_state(tsd, tprefix, activation, device)
        self.student = NativeMLP.from_sequential_state(ssd, "student", activation, device)
        self.loaded_teacher = True
        self._load_std(ssd)
        self.num_actions = self.student.dims[-1]
        if self.teacher.dims[-1] != self.num_actions:
            raise ValueError(f"the teacher ends in {self.teacher.dims[-1]} actions, the student in {self.num_actions}")
        self.seed, self._call = int(seed), 0
        self._mean = self._actions = self._teacher_actions = None
        self._sources = (tsd, ssd)

    def _check_teacher_memory(self, tprefix):
        pass

    def load_teacher(self, state_dict):
        """A new teacher image from a PPO state dict (`actor.*`) or a distillation one (`teacher.*`): the teacher half of
        `StudentTeacher.load_state_dict` (`student_teacher.py:125-144`).  The student, `std` and the call counter stay.  Returns the `teacher.*`
        entries it loaded (the trainers keep them for `state_dict()`)."""
        tprefix = "actor" if any("actor" in k for k in state_dict) else "teacher"
        self._check_teacher_memory(tprefix)
        entries = {"teacher." + k[len(tprefix) + 1:]: v.detach().clone() for k, v in state_dict.items() if k.startswith(tprefix + ".")}
        if not entries:
            raise ValueError("state_dict does not contain student or teacher parameters")
        teacher = NativeMLP.from_sequential_state(entries, "teacher", self._activation, str(self.device))
        if teacher.dims != self.teacher.dims:
            raise ValueError(f"the loaded teacher has layer widths {teacher.dims}, this policy's teacher {self.teacher.dims}")
        torch.cuda.synchronize(self.device)          # (the old image may still be read by a launch in flight)
        self.teacher = teacher
        self.loaded_teacher = True
        return entries

    def reset(self, dones=None, hidden_states=None):
        pass

    def get_hidden_states(self):
        return None

    def detach_hidden_states(self, dones=None):
        pass

    def _rows(self, n):
        super()._rows(n)
        self._teacher_actions = torch.empty(n, self.num_actions, device=self.device)

    def _launch(self, obs, tobs, deterministic=False):
        n = obs.shape[0]
        assert obs.shape == (n, self.student.dims[0]) and tobs.shape == (n, self.teacher.dims[0])
        self._rows(n)
        _check(self.student.lib.lg_distill_act(self.student.handle, self.teacher.handle, _ptr(obs), _ptr(tobs), n, _ptr(self.std), self.seed, self._call,
                                               int(deterministic), _ptr(self._actions), _ptr(self._mean), _ptr(self._teacher_actions), self.student._stream()),
               "lg_distill_act")

    def act_and_teach(self, obs, teacher_obs):
        """`Distillation.act` in one launch: (actions, privileged_actions)."""
        self._launch(self._f32(obs), self._f32(teacher_obs))
        return self._actions, self._teacher_actions

    def act(self, observations):
        """`StudentTeacher.act`: the same launch with the teacher on zeros (unused), so the draw for (seed, call, row) is `act_and_teach`'s."""
        obs = self._f32(observations)
        self._launch(obs, torch.zeros(obs.shape[0], self.teacher.dims[0], device=self.device))
        return self._actions

    def act_inference(self, observations):
        return self.student(observations)

    def evaluate(self, teacher_observations):
        return self.teacher(teacher_observations)


class NativeStudentTeacherRecurrent(NativeStudentTeacher):
    """`StudentTeacherRecurrent` (`modules/student_teacher_recurrent.py:15-100`): an `nn.LSTM` / `nn.GRU` `Memory` in front of the student and, with
    `teacher_recurrent`, in front of the teacher (`memory_s.rnn.*`, `memory_t.rnn.*`).  A recurrent teacher cannot come from a PPO checkpoint: the
    reference raises `NotImplementedError` there (`student_teacher.py:133-134`), and so does this class."""
    is_recurrent = True

    def __init__(self, state_dict, student_state_dict=None, activation="elu", rnn_type="lstm", teacher_recurrent=False, device="cuda:0", seed=0):
        self.teacher_recurrent = bool(teacher_recurrent)
        super().__init__(state_dict, student_state_dict, activation, device, seed)
        tsd, ssd = self._sources
        self.memory_s = NativeMemory.from_state(ssd, "memory_s", rnn_type, device)
        self.memory_t = NativeMemory.from_state(tsd, "memory_t", rnn_type, device) if self.teacher_recurrent else None
        if self.student.dims[0] != self.memory_s.hidden_size or (self.memory_t is not None and self.teacher.dims[0] != self.memory_t.hidden_size):
            raise ValueError("the MLPs of a StudentTeacherRecurrent take their memory's hidden state as input")

    def _check_teacher_memory(self, tprefix):
        if tprefix == "actor" and self.teacher_recurrent:
            raise NotImplementedError(TEACHER_MEMORY_MESSAGE)

    def reset(self, dones=None, hidden_states=None):
        """`StudentTeacherRecurrent.reset` (`:71-76`) with `Memory.reset(dones, hidden_states)` (`memory.py:35-51`): `dones` None installs
        `hidden_states` (None: forgets the state), else zeroes the done rows."""
        hs = hidden_states if hidden_states is not None else (None, None)
        for mem, h in ((self.memory_s, hs[0]), (self.memory_t, hs[1])):
            if mem is None:
                continue
            if dones is None and h is not None:
                mem.set_state(h)
            else:
                mem.reset(dones)

    def get_hidden_states(self):
        return self.memory_s.hidden_states, (self.memory_t.hidden_states if self.memory_t is not None else None)

    def _launch(self, obs, tobs, deterministic=False):
        n = obs.shape[0]
        mt = self.memory_t
        assert obs.shape == (n, self.memory_s.input_size) and tobs.shape == (n, mt.input_size if mt is not None else self.teacher.dims[0])
        self.memory_s.ensure_state(n)
        if mt is not None:
            mt.ensure_state(n)
        self._rows(n)
        tptrs = mt._ptrs() if mt is not None else (None, None)
        _check(self.student.lib.lg_distill_act_recurrent(self.memory_s.handle, self.student.handle, mt.handle if mt is not None else None, self.teacher.handle,
                                                         _ptr(obs), _ptr(tobs), n, _ptr(self.std), self.seed, self._call, int(deterministic),
                                                         *self.memory_s._ptrs(), *tptrs, None, _ptr(self._actions), _ptr(self._mean),
                                                         _ptr(self._teacher_actions), self.student._stream()), "lg_distill_act_recurrent")

    def act(self, observations):
        """Advances the STUDENT memory only (the teacher's waits for `evaluate`), then samples with the feed-forward launch on its output."""
        top = self.memory_s(observations)
        NativeStudentTeacher._launch(self, top, torch.zeros(top.shape[0], self.teacher.dims[0], device=self.device))
        return self._actions

    def act_inference(self, observations):
        return self.student(self.memory_s(observations))

    def evaluate(self, teacher_observations):
        return self.teacher(self.memory_t(teacher_observations) if self.memory_t is not None else teacher_observations)

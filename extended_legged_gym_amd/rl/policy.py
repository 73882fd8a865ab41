"""`NativeActorCritic`: the feed-forward `ActorCritic` of the vendored rsl_rl (`modules/actor_critic.py:16-136`) with its two
MLPs evaluated by `lg_mlp_forward` / `lg_policy_act` (include/lgpolicy.h): all layers of a network in one launch on the fp32
matrix cores, and `PPO.act` (`algorithms/ppo.py:147-159`: sample, value, log-prob, mean, sigma) as ONE launch instead of
~25.  Inference only: the weights come from a trained / initialised torch `ActorCritic` (its `state_dict`), gradients
stay in PyTorch.

`NativeActorCriticRecurrent`: rsl_rl's `ActorCriticRecurrent` (`modules/actor_critic_recurrent.py:16-85`: an `nn.LSTM` / `nn.GRU`
`Memory`, `networks/memory.py:16-51`, in front of each MLP) on `lg_rnn_step` / `lg_policy_act_recurrent`: one launch per memory layer
(both memories side by side) plus the `PPO.act` launch.  The hidden state lives in torch tensors the kernels update in place."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from extended_legged_gym_amd.native import load_library


def _lib():
    lib = load_library()
    if not getattr(lib, "_policy_declared", False):
        abi.declare_policy(lib)
        lib._policy_declared = True
    return lib


class NativeMLP:
    """nn.Sequential(Linear, act, ..., Linear) on the GPU.  `layers`: list of (weight (out, in), bias (out))."""

    def __init__(self, layers, activation="elu", device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("the policy kernels run on the GPU only (no CPU path)")
        self.lib, self.device = _lib(), dev
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
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.handle = self.lib.lg_mlp_create(L, (C.c_int32 * (L + 1))(*dims), wp, bp, abi.ACTIVATIONS[activation], index)
        if not self.handle:
            raise RuntimeError("lg_mlp_create failed: " + (self.lib.lg_mlp_last_error(None) or b"").decode())

    @classmethod
    def from_sequential_state(cls, state, prefix, activation="elu", device="cuda:0"):
        """Layers `prefix.0.weight`, `prefix.2.weight`, ... of an nn.Sequential state dict."""
        idx = sorted({int(k[len(prefix) + 1:].split(".")[0]) for k in state if k.startswith(prefix + ".") and k.endswith(".weight")})
        layers = [(state[f"{prefix}.{i}.weight"].detach().cpu().numpy(), state[f"{prefix}.{i}.bias"].detach().cpu().numpy()) for i in idx]
        return cls(layers, activation, device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __call__(self, x):
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        assert x.dim() == 2 and x.shape[1] == self.dims[0]
        y = torch.empty(x.shape[0], self.dims[-1], device=self.device)
        rc = self.lib.lg_mlp_forward(self.handle, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(y.data_ptr()), self._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_mlp_forward failed: " + (self.lib.lg_mlp_last_error(self.handle) or b"").decode())
        return y

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.lib.lg_mlp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeActorCritic:
    """Same surface as `ActorCritic` for rollout collection: `act`, `act_inference`, `evaluate`, `get_actions_log_prob`,
    `action_mean`, `action_std`, `entropy` (`actor_critic.py:96-136`)."""
    is_recurrent = False

    def __init__(self, state_dict, activation="elu", noise_std_type="scalar", device="cuda:0", seed=0):
        self.device = torch.device(device)
        self.actor = NativeMLP.from_sequential_state(state_dict, "actor", activation, device)
        self.critic = NativeMLP.from_sequential_state(state_dict, "critic", activation, device)
        self.noise_std_type = noise_std_type
        if noise_std_type == "scalar":
            self.std = state_dict["std"].detach().to(self.device, torch.float32).contiguous()
        elif noise_std_type == "log":
            self.std = torch.exp(state_dict["log_std"].detach().to(self.device, torch.float32)).contiguous()
        else:
            raise ValueError(f"Unknown standard deviation type: {noise_std_type}. Should be 'scalar' or 'log'")
        self.num_actions = self.actor.dims[-1]
        self.seed, self._call = int(seed), 0
        self._mean = self._actions = self._logp = self._values = None

    def reset(self, dones=None):
        pass

    def _run(self, obs, critic_obs, deterministic):
        lib = self.actor.lib
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        cobs = obs if critic_obs is None else critic_obs.to(device=self.device, dtype=torch.float32).contiguous()
        n = obs.shape[0]
        self._actions = torch.empty(n, self.num_actions, device=self.device)
        self._mean = torch.empty(n, self.num_actions, device=self.device)
        self._logp = torch.empty(n, device=self.device)
        self._values = torch.empty(n, self.critic.dims[-1], device=self.device)
        self._call += 1
        rc = lib.lg_policy_act(self.actor.handle, self.critic.handle, C.c_void_p(obs.data_ptr()), C.c_void_p(cobs.data_ptr()), n,
                               C.c_void_p(self.std.data_ptr()), self.seed, self._call, int(deterministic),
                               C.c_void_p(self._actions.data_ptr()), C.c_void_p(self._mean.data_ptr()),
                               C.c_void_p(self._logp.data_ptr()), C.c_void_p(self._values.data_ptr()), self.actor._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_policy_act failed: " + (lib.lg_mlp_last_error(self.actor.handle) or b"").decode())

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
        return (-((actions - self._mean) ** 2) / (2 * sd * sd) - torch.log(sd) - 0.9189385332046727).sum(dim=-1)

    @property
    def action_mean(self):
        return self._mean

    @property
    def action_std(self):
        return self.std.expand_as(self._mean)

    @property
    def entropy(self):
        return (0.5 + 0.9189385332046727 + torch.log(self.std)).sum().expand(self._mean.shape[0])


class NativeMemory:
    """One `Memory` (`networks/memory.py:16-51`) in inference mode.  `layers`: per RNN layer (weight_ih, weight_hh, bias_ih, bias_hh) in torch's
    layout; input width, hidden width and depth come from the shapes.  The state (`h`, and `c` for an LSTM; (L, n, H)) is allocated, zeroed,
    on the first step and again when the number of rows changes, as `Memory` does with `hidden_states = None`."""

    def __init__(self, layers, rnn_type="lstm", device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("the policy kernels run on the GPU only (no CPU path)")
        rnn_type = rnn_type.lower()
        if rnn_type not in abi.RNN_TYPES:
            raise ValueError(f"Unknown rnn_type: {rnn_type}. Should be 'lstm' or 'gru'")
        self.lib, self.device, self.rnn_type = _lib(), dev, rnn_type
        G = 4 if rnn_type == "lstm" else 3
        arrs = [[np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in layer] for layer in layers]
        self.num_layers, self.hidden_size, self.input_size = len(arrs), arrs[0][1].shape[1], arrs[0][0].shape[1]
        H = self.hidden_size
        for l, (wi, wh, bi, bh) in enumerate(arrs):
            assert wi.shape == (G * H, self.input_size if l == 0 else H) and wh.shape == (G * H, H) and bi.shape == bh.shape == (G * H,), \
                f"layer {l}: shapes do not belong to an nn.{rnn_type.upper()} of hidden size {H}"
        fp = C.POINTER(C.c_float)
        lists = [(fp * len(arrs))(*[layer[j].ctypes.data_as(fp) for layer in arrs]) for j in range(4)]
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.handle = self.lib.lg_rnn_create(abi.RNN_TYPES[rnn_type], self.num_layers, self.input_size, H, *lists, index)
        if not self.handle:
            raise RuntimeError("lg_rnn_create failed: " + (self.lib.lg_mlp_last_error(None) or b"").decode())
        self.h = self.c = None

    @classmethod
    def from_state(cls, state, prefix, rnn_type="lstm", device="cuda:0"):
        """Layers `prefix.rnn.weight_ih_l0`, ... of an `ActorCriticRecurrent` state dict."""
        L = len([k for k in state if k.startswith(prefix + ".rnn.weight_ih_l")])
        if L == 0:
            raise KeyError(f"no {prefix}.rnn.weight_ih_l0 in the state dict: not an ActorCriticRecurrent checkpoint")
        layers = [[state[f"{prefix}.rnn.{name}_l{l}"].detach().cpu().numpy() for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for l in range(L)]
        return cls(layers, rnn_type, device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def ensure_state(self, n):
        if self.h is None or self.h.shape[1] != n:
            self.h = torch.zeros(self.num_layers, n, self.hidden_size, device=self.device)
            self.c = torch.zeros_like(self.h) if self.rnn_type == "lstm" else None

    def _ptrs(self):
        return C.c_void_p(self.h.data_ptr()), C.c_void_p(self.c.data_ptr() if self.c is not None else None)

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
        rc = self.lib.lg_rnn_step(self.handle, C.c_void_p(x.data_ptr()), n, *self._ptrs(), C.c_void_p(reset.data_ptr() if reset is not None else None), None,
                                  self._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_rnn_step failed: " + (self.lib.lg_mlp_last_error(None) or b"").decode())
        return self.h[-1]

    def reset(self, dones=None):
        """`Memory.reset(dones)` (`memory.py:35-51`): None forgets the state; else rows with dones != 0 are zeroed."""
        if dones is None:
            self.h = self.c = None
        elif self.h is not None:
            d = dones.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
            assert d.shape[0] == self.h.shape[1]
            rc = self.lib.lg_rnn_reset_rows(self.handle, *self._ptrs(), C.c_void_p(d.data_ptr()), d.shape[0], self._stream())
            if rc != abi.LG_OK:
                raise RuntimeError("lg_rnn_reset_rows failed: " + (self.lib.lg_mlp_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "handle", None):
            torch.cuda.synchronize(self.device)
            self.lib.lg_rnn_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeActorCriticRecurrent(NativeActorCritic):
    """Same surface as `ActorCriticRecurrent` for rollout collection (`actor_critic_recurrent.py:62-85`): `act`, `act_inference`, `evaluate`,
    `reset(dones)`, `get_hidden_states`, and what `NativeActorCritic` has.  Built from an `ActorCriticRecurrent.state_dict()`
    (`memory_a.rnn.*`, `memory_c.rnn.*`, `actor.*`, `critic.*`, `std` / `log_std`).  The batch mode of `PPO.update` (`masks=` /
    `hidden_states=`) is not built."""
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
            raise NotImplementedError("masks= / hidden_states= (the batch mode of PPO.update) is PyTorch's job: the native policy collects rollouts only")

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def _run(self, obs, critic_obs, deterministic):
        lib = self.actor.lib
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        cobs = obs if critic_obs is None else critic_obs.to(device=self.device, dtype=torch.float32).contiguous()
        n = obs.shape[0]
        assert obs.shape[1] == self.memory_a.input_size and cobs.shape == (n, self.memory_c.input_size)
        self.memory_a.ensure_state(n)
        self.memory_c.ensure_state(n)
        self._actions = torch.empty(n, self.num_actions, device=self.device)
        self._mean = torch.empty(n, self.num_actions, device=self.device)
        self._logp = torch.empty(n, device=self.device)
        self._values = torch.empty(n, self.critic.dims[-1], device=self.device)
        self._call += 1
        rc = lib.lg_policy_act_recurrent(self.memory_a.handle, self.actor.handle, self.memory_c.handle, self.critic.handle, C.c_void_p(obs.data_ptr()),
                                         C.c_void_p(cobs.data_ptr()), n, C.c_void_p(self.std.data_ptr()), self.seed, self._call, int(deterministic),
                                         *self.memory_a._ptrs(), *self.memory_c._ptrs(), None, C.c_void_p(self._actions.data_ptr()),
                                         C.c_void_p(self._mean.data_ptr()), C.c_void_p(self._logp.data_ptr()), C.c_void_p(self._values.data_ptr()),
                                         self.actor._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_policy_act_recurrent failed: " + (lib.lg_mlp_last_error(self.actor.handle) or b"").decode())

    def act(self, observations, masks=None, hidden_states=None):
        """`ActorCriticRecurrent.act`: advances the ACTOR memory only (the critic's waits for `evaluate`); samples with `lg_policy_act` on its
        output, so the draw for (seed, call, row) is the one `act_and_evaluate` makes.  The critic MLP of that launch runs on zeros, unused."""
        self._no_batch_mode(masks, hidden_states)
        lib = self.actor.lib
        top = self.memory_a(observations)
        n = top.shape[0]
        idle = torch.zeros(n, self.critic.dims[0], device=self.device)
        self._actions = torch.empty(n, self.num_actions, device=self.device)
        self._mean = torch.empty(n, self.num_actions, device=self.device)
        self._logp = torch.empty(n, device=self.device)
        unused = torch.empty(n, self.critic.dims[-1], device=self.device)
        self._call += 1
        rc = lib.lg_policy_act(self.actor.handle, self.critic.handle, C.c_void_p(top.data_ptr()), C.c_void_p(idle.data_ptr()), n,
                               C.c_void_p(self.std.data_ptr()), self.seed, self._call, 0, C.c_void_p(self._actions.data_ptr()),
                               C.c_void_p(self._mean.data_ptr()), C.c_void_p(self._logp.data_ptr()), C.c_void_p(unused.data_ptr()), self.actor._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_policy_act failed: " + (lib.lg_mlp_last_error(self.actor.handle) or b"").decode())
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


class NativeStudentTeacher:
    """Same surface as rsl_rl's `StudentTeacher` (`modules/student_teacher.py:75-152`) for collection with `Distillation` (`distillation.py:89-105`)
    and for `get_inference_policy`: `act`, `act_inference`, `evaluate`, `reset`, `get_hidden_states`, `action_mean`, `action_std`, `loaded_teacher`;
    `act_and_teach(obs, teacher_obs)` is `Distillation.act` as ONE launch (`lg_distill_act`).  Inference only: `Distillation.update` trains a torch
    `StudentTeacher` whose state dict builds this object."""
    is_recurrent = False

    def __init__(self, state_dict, student_state_dict=None, activation="elu", device="cuda:0", seed=0):
        self.device = torch.device(device)
        tsd, ssd, tprefix, self.resumed = _split_distillation_state(state_dict, student_state_dict)
        self._check_teacher_memory(tprefix)
        self.teacher = NativeMLP.from_sequential_state(tsd, tprefix, activation, device)
        self.student = NativeMLP.from_sequential_state(ssd, "student", activation, device)
        self.loaded_teacher = True
        self.std = ssd["std"].detach().to(self.device, torch.float32).contiguous()
        self.num_actions = self.student.dims[-1]
        if self.teacher.dims[-1] != self.num_actions:
            raise ValueError(f"the teacher ends in {self.teacher.dims[-1]} actions, the student in {self.num_actions}")
        self.seed, self._call = int(seed), 0
        self._mean = self._actions = self._teacher_actions = None
        self._sources = (tsd, ssd)

    def _check_teacher_memory(self, tprefix):
        pass

    def reset(self, dones=None, hidden_states=None):
        pass

    def get_hidden_states(self):
        return None

    def detach_hidden_states(self, dones=None):
        pass

    def _rows(self, n):
        self._actions = torch.empty(n, self.num_actions, device=self.device)
        self._mean = torch.empty(n, self.num_actions, device=self.device)
        self._teacher_actions = torch.empty(n, self.num_actions, device=self.device)
        self._call += 1

    def _launch(self, obs, tobs, deterministic=False):
        lib = self.student.lib
        n = obs.shape[0]
        assert obs.shape == (n, self.student.dims[0]) and tobs.shape == (n, self.teacher.dims[0])
        self._rows(n)
        rc = lib.lg_distill_act(self.student.handle, self.teacher.handle, C.c_void_p(obs.data_ptr()), C.c_void_p(tobs.data_ptr()), n,
                                C.c_void_p(self.std.data_ptr()), self.seed, self._call, int(deterministic), C.c_void_p(self._actions.data_ptr()),
                                C.c_void_p(self._mean.data_ptr()), C.c_void_p(self._teacher_actions.data_ptr()), self.student._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_distill_act failed: " + (lib.lg_mlp_last_error(self.student.handle) or b"").decode())

    def _f32(self, x):
        return x.to(device=self.device, dtype=torch.float32).contiguous()

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

    @property
    def action_mean(self):
        return self._mean

    @property
    def action_std(self):
        return self.std.expand_as(self._mean)

    @property
    def entropy(self):
        return (0.5 + 0.9189385332046727 + torch.log(self.std)).sum().expand(self._mean.shape[0])


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
                parts = h if isinstance(h, (tuple, list)) else (h,)
                mem.h = parts[0].detach().to(self.device, torch.float32).clone().contiguous()
                mem.c = parts[1].detach().to(self.device, torch.float32).clone().contiguous() if mem.rnn_type == "lstm" else None
            else:
                mem.reset(dones)

    def get_hidden_states(self):
        return self.memory_s.hidden_states, (self.memory_t.hidden_states if self.memory_t is not None else None)

    def _launch(self, obs, tobs, deterministic=False):
        lib = self.student.lib
        n = obs.shape[0]
        mt = self.memory_t
        assert obs.shape == (n, self.memory_s.input_size) and tobs.shape == (n, mt.input_size if mt is not None else self.teacher.dims[0])
        self.memory_s.ensure_state(n)
        if mt is not None:
            mt.ensure_state(n)
        self._rows(n)
        tptrs = mt._ptrs() if mt is not None else (None, None)
        rc = lib.lg_distill_act_recurrent(self.memory_s.handle, self.student.handle, mt.handle if mt is not None else None, self.teacher.handle,
                                          C.c_void_p(obs.data_ptr()), C.c_void_p(tobs.data_ptr()), n, C.c_void_p(self.std.data_ptr()), self.seed, self._call,
                                          int(deterministic), *self.memory_s._ptrs(), *tptrs, None, C.c_void_p(self._actions.data_ptr()),
                                          C.c_void_p(self._mean.data_ptr()), C.c_void_p(self._teacher_actions.data_ptr()), self.student._stream())
        if rc != abi.LG_OK:
            raise RuntimeError("lg_distill_act_recurrent failed: " + (lib.lg_mlp_last_error(self.student.handle) or b"").decode())

    def act(self, observations):
        """Advances the STUDENT memory only (the teacher's waits for `evaluate`), then samples with the feed-forward launch on its output."""
        top = self.memory_s(observations)
        NativeStudentTeacher._launch(self, top, torch.zeros(top.shape[0], self.teacher.dims[0], device=self.device))
        return self._actions

    def act_inference(self, observations):
        return self.student(self.memory_s(observations))

    def evaluate(self, teacher_observations):
        return self.teacher(self.memory_t(teacher_observations) if self.memory_t is not None else teacher_observations)

"""`NativeDistillation`: `Distillation.update` of the vendored rsl_rl (`algorithms/distillation.py:107-153`, batches in time order as
`storage/rollout_storage.py:170-182`) for a feed-forward `NativeStudentTeacher`, on the library's training kernels (include/lgdistill.h): every
`gradient_length` consecutive steps are one batch through forward with saved activations, the behaviour loss, backward, the optional grad-norm clip
and Adam on the device.  Only the student moves; its weights stay on the device and are updated in place, in the tiled images `policy.act*` and
`collect_distillation` read: collect -> update -> collect never returns to the host for parameters."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from .policy import NativeStudentTeacher, _ptr
from .ppo import _sequential_layers
from .trainer import _NativeTrainer


class NativeDistillation(_NativeTrainer):
    """rsl_rl's `Distillation` for a feed-forward `NativeStudentTeacher`, with its names and defaults.  `state_dict`: the `StudentTeacher` state dict
    `policy` was built from (`student.*`, `teacher.*`, `std`); `student.*` seeds the fp32 master parameters.  After `update`, the same `policy`
    object acts with the new student; nothing is rebuilt."""
    _destroy = "lg_distill_train_destroy"
    _prefix = "lg_distill_train_"
    _declare = staticmethod(abi.declare_distill_train)

    def __init__(self, policy, state_dict, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 multi_gpu_cfg=None, max_rows=None):
        if loss_type not in abi.DISTILL_LOSSES:
            raise ValueError(f"Unknown loss type: {loss_type}. Supported types are: mse, huber")
        if getattr(policy, "is_recurrent", False):
            raise NotImplementedError("a recurrent student (NativeStudentTeacherRecurrent: truncated BPTT) is not built in the native update")
        if multi_gpu_cfg:
            raise NotImplementedError("multi_gpu_cfg is not built in the native update")
        if not isinstance(policy, NativeStudentTeacher):
            raise TypeError("NativeDistillation trains a NativeStudentTeacher")
        self._open_trainer(policy.device)
        self.policy = policy
        self.num_learning_epochs, self.gradient_length = int(num_learning_epochs), int(gradient_length)
        self.learning_rate, self.max_grad_norm, self.loss_type = float(learning_rate), max_grad_norm, loss_type
        self.max_rows = max_rows
        self._idx, self._layers = _sequential_layers(state_dict, "student")
        self._shapes = []
        for i, (w, b) in zip(self._idx, self._layers):
            self._shapes += [(f"student.{i}.weight", w.shape), (f"student.{i}.bias", b.shape)]
        self._rest = {k: v.detach().clone() for k, v in state_dict.items() if not k.startswith("student.")}          # teacher.*, std: never written
        self._stats = torch.zeros(3, dtype=torch.float64, device=self.device)
        self.num_updates = 0
        self._group_steps = self._last_steps = 0          # steps of the last group / of the last update
        self.optimizer_steps = self.grad_norm = None
        if max_rows is not None:
            self._create(int(max_rows))

    # ---- handle
    def _make_handle(self, max_rows):
        fp = C.POINTER(C.c_float)
        ws = (fp * len(self._layers))(*[w.ctypes.data_as(fp) for w, _ in self._layers])
        bs = (fp * len(self._layers))(*[b.ctypes.data_as(fp) for _, b in self._layers])
        return self._fn("create")(self.policy.student.handle, ws, bs, self.learning_rate, max_rows)

    def _hyper(self):
        return abi.lg_distill_train_hyper(abi.DISTILL_LOSSES[self.loss_type], float(self.max_grad_norm) if self.max_grad_norm else 0.0)

    def _rows(self, rows):
        """The (T, N, .) observations and targets of a `collect_distillation` dict, contiguous fp32 on the device."""
        obs = rows["observations"].to(device=self.device, dtype=torch.float32).contiguous()
        tgt = rows["privileged_actions"].to(device=self.device, dtype=torch.float32).contiguous()
        assert obs.dim() == 3 and obs.shape[2] == self.policy.student.dims[0] and tgt.shape == (obs.shape[0], obs.shape[1], self.policy.num_actions)
        return obs, tgt, obs.shape[0], obs.shape[1]

    # ---- training
    def group(self, rows, first_step, num_steps):
        """One optimiser step on the sum of the losses of `num_steps` consecutive steps; step s reads time index (first_step + s) mod T."""
        obs, tgt, T, N = self._rows(rows)
        self._ensure(max(int(num_steps), 1) * N)
        hyper = self._hyper()
        self._call("group", _ptr(obs), _ptr(tgt), T, N, int(first_step), int(num_steps), C.byref(hyper))
        self._group_steps = int(num_steps)

    def update(self, rows):
        """`Distillation.update` on the dict `collect_distillation` returns: the loss dict {"behavior": mean over the E * T steps}.  The number of
        optimiser steps and the last gradient norm arrive with the same device-to-host copy (`optimizer_steps`, `grad_norm`)."""
        self.num_updates += 1
        obs, tgt, T, N = self._rows(rows)
        self._ensure(self.gradient_length * N)
        hyper = self._hyper()
        self._call("update", _ptr(obs), _ptr(tgt), T, N, self.num_learning_epochs, self.gradient_length, C.byref(hyper), _ptr(self._stats))
        st = self._stats.cpu().tolist()
        self._last_steps = self.num_learning_epochs * T
        if self._last_steps >= self.gradient_length:
            self._group_steps = self.gradient_length
        self.optimizer_steps, self.grad_norm = int(st[1]), st[2]
        return {"behavior": st[0]}

    # ---- what the device holds (the checkpoint methods are `_NativeTrainer`'s; `state_dict()` is a `StudentTeacher` state dict: `student.*` as
    # trained, `teacher.*` and `std` as given)
    def gradients(self):
        """The last group's gradients before the clip (dict in the state dict's names), the global norm, and its per-step losses."""
        self._need_handle()
        g, norm, losses = np.empty(self.num_parameters, np.float32), C.c_float(), np.empty(self._group_steps, np.float32)
        self._call("gradients", g.ctypes.data, C.addressof(norm), losses.ctypes.data, losses.size)
        return self._split(g), norm.value, [float(x) for x in losses]

    def forward_outputs(self, rows):
        """The student's outputs (rows, A) of the last group's forward pass, step-major."""
        self._need_handle()
        out = np.empty((rows, self.policy.num_actions), np.float32)
        self._call("forward_outputs", out.ctypes.data)
        return torch.from_numpy(out)

    def load_teacher(self, state_dict):
        """Swaps the teacher (`policy.load_teacher`: `actor.*` of a PPO checkpoint or `teacher.*`) in the policy's image and in the `teacher.*`
        entries `state_dict()` returns; nothing that is trained moves."""
        self._rest.update(self.policy.load_teacher(state_dict))

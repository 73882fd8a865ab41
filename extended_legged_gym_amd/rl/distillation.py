"""`NativeDistillation`: `Distillation.update` of the vendored rsl_rl (`algorithms/distillation.py:107-153`, batches in time order as
`storage/rollout_storage.py:170-182`) for a feed-forward `NativeStudentTeacher`, on the library's training kernels (include/lgdistill.h): every
`gradient_length` consecutive steps are one batch through forward with saved activations, the behaviour loss, backward, the optional grad-norm clip
and Adam on the device.  Only the student moves; its weights stay on the device and are updated in place, in the tiled images `policy.act*` and
`collect_distillation` read: collect -> update -> collect never returns to the host for parameters."""
import ctypes as C

import torch

from extended_legged_gym_amd import abi
from .policy import NativeStudentTeacher
from .ppo import _sequential_layers
from .trainer import _NativeSequenceTrainer


class NativeDistillation(_NativeSequenceTrainer):
    """rsl_rl's `Distillation` for a feed-forward `NativeStudentTeacher`, with its names and defaults.  `state_dict`: the `StudentTeacher` state dict
    `policy` was built from (`student.*`, `teacher.*`, `std`); `student.*` seeds the fp32 master parameters.  After `update`, the same `policy`
    object acts with the new student; nothing is rebuilt."""
    _destroy = "lg_distill_train_destroy"
    _prefix = "lg_distill_train_"
    _unit = "distill_train"
    _hyper_type, _losses, _loss_name = abi.lg_distill_train_hyper, abi.DISTILL_LOSSES, "behavior"
    _norm_needs_step = False
    _group_has_train = False

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
        self._out_w = policy.num_actions
        self.optimizer_steps = self.grad_norm = None
        if max_rows is not None:
            self._create(int(max_rows))

    # ---- handle
    def _make_handle(self, max_rows):
        fp = C.POINTER(C.c_float)
        ws = (fp * len(self._layers))(*[w.ctypes.data_as(fp) for w, _ in self._layers])
        bs = (fp * len(self._layers))(*[b.ctypes.data_as(fp) for _, b in self._layers])
        return self._fn("create")(self.policy.student.handle, ws, bs, self.learning_rate, max_rows)

    def _rows(self, rows):
        """The (T, N, .) observations and targets of a `collect_distillation` dict, contiguous fp32 on the device."""
        obs = rows["observations"].to(device=self.device, dtype=torch.float32).contiguous()
        tgt = rows["privileged_actions"].to(device=self.device, dtype=torch.float32).contiguous()
        assert obs.dim() == 3 and obs.shape[2] == self.policy.student.dims[0] and tgt.shape == (obs.shape[0], obs.shape[1], self.policy.num_actions)
        return obs, tgt, obs.shape[0], obs.shape[1]

    # ---- training (`update`, `gradients` and `forward_outputs(rows)` are `_NativeSequenceTrainer`'s; the checkpoint methods `_NativeTrainer`'s;
    # `state_dict()` is a `StudentTeacher` state dict: `student.*` as trained, `teacher.*` and `std` as given)
    def group(self, rows, first_step, num_steps):
        """One optimiser step on the sum of the losses of `num_steps` consecutive steps; step s reads time index (first_step + s) mod T."""
        super().group(rows, first_step, num_steps)

    def _after_update(self, N):
        """csrc/lg_distill_train.hip, distill_steps: `if (train) p->last_steps = nsteps;` -- a forward-only remainder leaves the last group's."""
        rem = self._last_steps % self.gradient_length
        if self._last_steps >= self.gradient_length:
            self._group_steps = self.gradient_length
        self._last_rows = (rem if rem else self.gradient_length) * N

    def load_teacher(self, state_dict):
        """Swaps the teacher (`policy.load_teacher`: `actor.*` of a PPO checkpoint or `teacher.*`) in the policy's image and in the `teacher.*`
        entries `state_dict()` returns; nothing that is trained moves."""
        self._rest.update(self.policy.load_teacher(state_dict))

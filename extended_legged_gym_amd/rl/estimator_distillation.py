"""`NativeEstimatorDistillation`: `EstimatorDistillation.update` of the vendored rsl_rl (`algorithms/distillation.py:277-332`, through
`runners/terrain_estimator_runner.py`) for a `NativeTerrainEstimator`, on the library's training kernels (include/lgestimator_train.h): every
`gradient_length` consecutive steps are one batch through the encoder's forward with saved maps, the memory through time, the decoder, the loss,
truncated BPTT, the convolutions' data and weight gradients, the optional grad-norm clip and Adam on the device.  The weights stay on the device and
are updated in place, in the images `act_inference` and `collect_estimation` read: collect -> update -> collect never returns to the host for
parameters."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from .estimator import NativeTerrainEstimator, parse_estimator_state
from .policy import _NativeHandle, _lib, _ptr


def _estimator_train_lib():
    lib = _lib()
    if not getattr(lib, "_estimator_train_declared", False):
        abi.declare_estimator_train(lib)
        lib._estimator_train_declared = True
    return lib


class NativeEstimatorDistillation(_NativeHandle):
    """rsl_rl's `EstimatorDistillation` for a `NativeTerrainEstimator`, with its names and defaults.  `state_dict`: the `TerrainEstimator` state
    dict `estimator` was built from; it seeds the fp32 master parameters.  After `update`, the same `estimator` object predicts with the new
    weights; nothing is rebuilt, and its live inference state is not touched: the trainer owns the state it carries from update to update
    (`get_hidden_states` / `set_hidden_states`)."""
    _destroy = "lg_estimator_train_destroy"

    def __init__(self, estimator, state_dict, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 use_dones=False, multi_gpu_cfg=None, max_rows=None):
        if loss_type not in abi.ESTIMATOR_LOSSES:
            raise ValueError(f"Unknown loss type: {loss_type}. Supported types are: mse, huber, l1")
        if multi_gpu_cfg:
            raise NotImplementedError("multi_gpu_cfg is not built in the native update")
        if getattr(estimator, "precision", "fp32") != "fp32":
            raise NotImplementedError("an estimator with encoder_precision=\"bf16\" is not trained by the native update: train an fp32 estimator, then build a "
                                      "bf16 one from state_dict()")
        if not isinstance(estimator, NativeTerrainEstimator):
            raise TypeError("NativeEstimatorDistillation trains a NativeTerrainEstimator")
        self._open(estimator.device, "training")
        self.lib = _estimator_train_lib()
        self.estimator = estimator
        self.num_learning_epochs, self.gradient_length = int(num_learning_epochs), int(gradient_length)
        self.learning_rate, self.max_grad_norm, self.loss_type, self.use_dones = float(learning_rate), max_grad_norm, loss_type, bool(use_dones)
        self.max_rows = max_rows
        spec = parse_estimator_state(state_dict, estimator.depth_image_shape, estimator.proprio_dim, estimator.spec["memory_type"])
        self._spec = spec
        L = spec["memory_num_layers"]
        dec_idx = sorted({int(k.split(".")[1]) for k in (state_dict.get("model_state_dict", state_dict)) if k.startswith("decoder.") and k.endswith(".weight")})
        # the flat order: the module's own state_dict() order
        self._shapes = []
        for i, (w, b) in zip((0, 2, 4, 6, 10, 12), spec["encoder"]):
            self._shapes += [(f"depth_encoder.{i}.weight", w.shape), (f"depth_encoder.{i}.bias", b.shape)]
        self._shapes += [("combination_mlp.0.weight", spec["combine"][0].shape), ("combination_mlp.0.bias", spec["combine"][1].shape)]
        for l in range(L):
            for name, a in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), spec["memory"][l]):
                self._shapes.append((f"memory.rnn.{name}_l{l}", a.shape))
        for i, (w, b) in zip(dec_idx, spec["decoder"]):
            self._shapes += [(f"decoder.{i}.weight", w.shape), (f"decoder.{i}.bias", b.shape)]
        self.handle = None
        self._stats = torch.zeros(3, dtype=torch.float64, device=self.device)
        self.num_updates = 0
        self._group_steps = self._last_steps = self._last_rows = 0
        self.optimizer_steps, self.last_grad_norm = None, 0.0          # as the reference: 0.0 until a step is taken
        if max_rows is not None:
            self._create(int(max_rows))

    # ---- handle
    def _create(self, max_rows):
        spec, fp = self._spec, C.POINTER(C.c_float)

        def plist(arrays):
            return (fp * len(arrays))(*[a.ctypes.data_as(fp) for a in arrays])

        q = abi.lg_estimator_train_params(
            plist([w for w, _ in spec["encoder"]]), plist([b for _, b in spec["encoder"]]), spec["combine"][0].ctypes.data_as(fp), spec["combine"][1].ctypes.data_as(fp),
            plist([m[0] for m in spec["memory"]]), plist([m[1] for m in spec["memory"]]), plist([m[2] for m in spec["memory"]]), plist([m[3] for m in spec["memory"]]),
            plist([w for w, _ in spec["decoder"]]), plist([b for _, b in spec["decoder"]]))
        state = self.optimizer_state() if self.handle else None
        carry = self.get_hidden_states() if self.handle else None
        self.close()
        torch.cuda.synchronize(self.device)
        est = self.estimator
        self._created(self.lib.lg_estimator_train_create(est.encoder.handle, est.combine.handle, est.memory.handle, est.decoder.handle, C.byref(q), self.learning_rate,
                                                         max_rows), "lg_estimator_train_create")
        self.max_rows = max_rows
        self.num_parameters = int(self.lib.lg_estimator_train_parameter_count(self.handle))
        if state is not None:
            self.load_optimizer_state(state)
        if carry is not None:
            self.set_hidden_states(carry)

    def _ensure(self, rows):
        if self.handle is None or rows > self.max_rows:
            self._create(rows)

    def _need_handle(self):
        if self.handle is None:
            self._create(1)

    def _hyper(self):
        return abi.lg_estimator_train_hyper(abi.ESTIMATOR_LOSSES[self.loss_type], float(self.max_grad_norm) if self.max_grad_norm else 0.0, int(self.use_dones))

    def _rows(self, rows):
        """The (T, N, .) tensors of a `collect_estimation` dict, contiguous fp32 on the device."""
        est = self.estimator
        depth = rows["depth_images"]
        if depth.dim() == 5:
            depth = depth[:, :, -1]
        depth = depth.to(device=self.device, dtype=torch.float32).contiguous()
        T, N = depth.shape[:2]
        prop = rows["proprio_data"].to(device=self.device, dtype=torch.float32).contiguous()
        tgt = rows["raycast_targets"].to(device=self.device, dtype=torch.float32).contiguous()
        assert depth.shape == (T, N, *est.depth_image_shape) and prop.shape == (T, N, est.proprio_dim) and tgt.shape == (T, N, est.num_raycast_outputs)
        dones = None
        if self.use_dones:
            dones = rows["dones"].to(device=self.device, dtype=torch.float32).contiguous().view(T, N)
        return depth, prop, tgt, dones, T, N

    # ---- training
    def group(self, rows, first_step, num_steps, train=True):
        """One optimiser step on the sum of the losses of `num_steps` consecutive steps; step s reads time index (first_step + s) mod T.  A step
        with time index 0 enters with the carried state, the first step otherwise with the state the last step run left.  `train=False`: forward
        and losses only (the remainder of an update)."""
        depth, prop, tgt, dones, T, N = self._rows(rows)
        self._ensure(max(int(num_steps), 1) * N)
        hyper = self._hyper()
        self._check(self.lib.lg_estimator_train_group(self.handle, _ptr(depth), _ptr(prop), _ptr(tgt), _ptr(dones), T, N, int(first_step), int(num_steps),
                                                      1 if train else 0, C.byref(hyper), self._stream()), "lg_estimator_train_group")
        self._group_steps, self._last_rows = int(num_steps), int(num_steps) * N

    def update(self, rows):
        """`EstimatorDistillation.update` on the dict `collect_estimation` returns: the loss dict {"estimation": mean over the E * T steps}.  The
        number of optimiser steps and the last gradient norm arrive with the same device-to-host copy (`optimizer_steps`, `last_grad_norm`)."""
        self.num_updates += 1
        depth, prop, tgt, dones, T, N = self._rows(rows)
        self._ensure(self.gradient_length * N)
        hyper = self._hyper()
        self._check(self.lib.lg_estimator_train_update(self.handle, _ptr(depth), _ptr(prop), _ptr(tgt), _ptr(dones), T, N, self.num_learning_epochs,
                                                       self.gradient_length, C.byref(hyper), _ptr(self._stats), self._stream()), "lg_estimator_train_update")
        st = self._stats.cpu().tolist()
        self._last_steps = self.num_learning_epochs * T
        rem = self._last_steps % self.gradient_length
        self._group_steps = rem if rem else self.gradient_length
        self._last_rows = self._group_steps * N
        self.optimizer_steps = int(st[1])
        if self.optimizer_steps:
            self.last_grad_norm = st[2]
        return {"estimation": st[0]}

    def set_learning_rate(self, learning_rate):
        self.learning_rate = float(learning_rate)
        if self.handle:
            self._check(self.lib.lg_estimator_train_set_learning_rate(self.handle, self.learning_rate, self._stream()), "lg_estimator_train_set_learning_rate")

    def workspace_bytes(self):
        self._need_handle()
        return int(self.lib.lg_estimator_train_workspace_bytes(self.handle))

    # ---- the carried state
    def get_hidden_states(self, running=False):
        """The state the next update's epochs start from (`last_hidden_states`): `h` (L, N, H) for a GRU, `(h, c)` for an LSTM, None before the
        first update.  `running=True`: the state after the last step run instead (what a loop of `group` calls hands to `set_hidden_states`)."""
        if self.handle is None:
            return None
        N = int(self.lib.lg_estimator_train_get_carry(self.handle, None, None, 0, 0, self._stream()))
        if N <= 0:
            return None
        L, H = self._spec["memory_num_layers"], self._spec["memory_hidden_size"]
        lstm = self._spec["memory_type"] == "lstm"
        h, c = np.empty((L, N, H), np.float32), (np.empty((L, N, H), np.float32) if lstm else None)
        got = self.lib.lg_estimator_train_get_carry(self.handle, h.ctypes.data, c.ctypes.data if lstm else None, N, 1 if running else 0, self._stream())
        if got != N:
            self._check(int(got), "lg_estimator_train_get_carry")
        h = torch.from_numpy(h).to(self.device)
        return (h, torch.from_numpy(c).to(self.device)) if lstm else h

    def set_hidden_states(self, hidden_states):
        """Installs the carried state (None: forgets it; the next update starts from zeros, with any number of rows)."""
        self._need_handle()
        if hidden_states is None:
            self._check(self.lib.lg_estimator_train_reset_carry(self.handle, self._stream()), "lg_estimator_train_reset_carry")
            return
        parts = hidden_states if isinstance(hidden_states, (tuple, list)) else (hidden_states,)
        arrs = [np.ascontiguousarray(p.detach().cpu().numpy(), dtype=np.float32) for p in parts]
        L, H = self._spec["memory_num_layers"], self._spec["memory_hidden_size"]
        N = arrs[0].shape[1]
        assert all(a.shape == (L, N, H) for a in arrs)
        self._ensure(N)
        self._check(self.lib.lg_estimator_train_set_carry(self.handle, arrs[0].ctypes.data, arrs[1].ctypes.data if len(arrs) > 1 else None, N, self._stream()),
                    "lg_estimator_train_set_carry")

    # ---- what the device holds
    def _split(self, flat):
        out, off = {}, 0
        for name, shape in self._shapes:
            cnt = int(np.prod(shape))
            out[name] = torch.from_numpy(flat[off:off + cnt].reshape(shape).copy()); off += cnt
        return out

    def _join(self, tensors):
        flat = np.ascontiguousarray(np.concatenate([tensors[name].detach().cpu().numpy().reshape(-1) for name, _ in self._shapes]), dtype=np.float32)
        assert flat.size == self.num_parameters
        return flat

    def gradients(self):
        """The last group's gradients before the clip (dict in the state dict's names), the global norm, and its per-step losses."""
        self._need_handle()
        g, norm, losses = np.empty(self.num_parameters, np.float32), C.c_float(), np.empty(self._group_steps, np.float32)
        self._check(self.lib.lg_estimator_train_gradients(self.handle, g.ctypes.data, C.addressof(norm), losses.ctypes.data, losses.size, self._stream()),
                    "lg_estimator_train_gradients")
        return self._split(g), norm.value, [float(x) for x in losses]

    def forward_outputs(self):
        """The predictions (rows, R) of the last group's (or remainder's) forward pass, step-major."""
        self._need_handle()
        out = np.empty((self._last_rows, self.estimator.num_raycast_outputs), np.float32)
        self._check(self.lib.lg_estimator_train_forward_outputs(self.handle, out.ctypes.data, self._stream()), "lg_estimator_train_forward_outputs")
        return torch.from_numpy(out)

    def step_losses(self):
        """The E * T fp32 step losses of the last `update`."""
        self._need_handle()
        out = np.empty(self._last_steps, np.float32)
        self._check(self.lib.lg_estimator_train_step_losses(self.handle, out.ctypes.data, out.size, self._stream()), "lg_estimator_train_step_losses")
        return torch.from_numpy(out)

    def state_dict(self):
        """A `TerrainEstimator` state dict as trained: `NativeTerrainEstimator`, `TerrainEstimatorTorch` and the reference's module load it."""
        self._need_handle()
        flat = np.empty(self.num_parameters, np.float32)
        self._check(self.lib.lg_estimator_train_get_parameters(self.handle, flat.ctypes.data, self._stream()), "lg_estimator_train_get_parameters")
        return self._split(flat)

    def optimizer_state(self):
        """Masters, both Adam moments, the step count and the learning rate."""
        self._need_handle()
        bufs = [np.empty(self.num_parameters, np.float32) for _ in range(3)]
        step, lr = C.c_int64(), C.c_double()
        self._check(self.lib.lg_estimator_train_get_state(self.handle, *[b.ctypes.data for b in bufs], C.byref(step), C.byref(lr), self._stream()),
                    "lg_estimator_train_get_state")
        return dict(parameters=self._split(bufs[0]), exp_avg=self._split(bufs[1]), exp_avg_sq=self._split(bufs[2]), step=step.value, learning_rate=lr.value)

    def load_optimizer_state(self, state):
        self._need_handle()
        bufs = [self._join(state[k]) for k in ("parameters", "exp_avg", "exp_avg_sq")]
        self._check(self.lib.lg_estimator_train_set_state(self.handle, *[b.ctypes.data for b in bufs], int(state["step"]), float(state["learning_rate"]),
                                                          self._stream()), "lg_estimator_train_set_state")
        self.learning_rate = float(state["learning_rate"])

    def load_state_dict(self, state_dict):
        """New parameters (a `TerrainEstimator` state dict); the moments, the step count and the learning rate stay."""
        state = self.optimizer_state()
        state["parameters"] = state_dict
        self.load_optimizer_state(state)

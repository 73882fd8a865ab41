"""`_NativeTrainer`: what the owners of a native trainer handle share (`NativePPO` and its two subclasses, `NativeDistillation`,
`NativeRecurrentDistillation`, `NativeEstimatorDistillation`).  Every trainer's header exports the same group of entry points under its own prefix
(`abi._declare_trainer_group`); this is their one Python side: the flat parameter layout, the checkpoint methods, the handle that regrows when a
call brings more rows than it was built for, and the carried memory state of the two trainers that keep one."""
import ctypes as C

import numpy as np
import torch

from .policy import _NativeHandle, _lib, _ptr


def _declared(declare):
    """The library with the prototypes of `declare` (an `abi.declare_*`) set, once."""
    lib, flag = _lib(), "_" + declare.__name__ + "d"
    if not getattr(lib, flag, False):
        declare(lib)
        setattr(lib, flag, True)
    return lib


class _NativeTrainer(_NativeHandle):
    """A subclass names its header (`_prefix`, `_declare`), lists the trained tensors as (name, shape) pairs in the flat order of the library's
    parameter vector (`_shapes`), keeps the state dict's untrained entries in `_rest`, and builds its handle in `_make_handle(max_rows)`."""
    _prefix = None           # "lg_ppo_", ...: the entry points of the class's header
    _declare = None          # staticmethod(abi.declare_*) of that header
    _rest = {}               # the state dict's entries that are never trained, returned by `state_dict()` as given
    _carry = None            # (layers, hidden size, is_lstm) of the memory whose state the trainer carries from update to update; None: no memory
    _carry_on_device = False          # the library's carry calls take device tensors (else host arrays)
    handle = None

    def _open_trainer(self, device):
        self._open(device, "training")
        self.lib = _declared(self._declare)

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _call(self, name, *args):
        """`<prefix><name>(handle, *args, stream)`, checked."""
        self._check(self._fn(name)(self.handle, *args, self._stream()), self._prefix + name)

    # ---- handle
    def _create(self, max_rows, **kw):
        """(Re)builds the handle for `max_rows` rows; what the old one had learnt and carried moves to the new one."""
        state = self.optimizer_state() if self.handle else None
        carry = self.get_hidden_states() if self.handle and self._carry else None
        self.close()
        torch.cuda.synchronize(self.device)
        self._created(self._make_handle(max_rows, **kw), self._prefix + "create")
        self.max_rows = max_rows
        self.num_parameters = int(self._fn("parameter_count")(self.handle))
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

    def set_learning_rate(self, learning_rate):
        self.learning_rate = float(learning_rate)
        if self.handle:
            self._call("set_learning_rate", self.learning_rate)

    def workspace_bytes(self):
        """Device bytes the handle owns (the trainers whose header has the call)."""
        self._need_handle()
        return int(self._fn("workspace_bytes")(self.handle))

    # ---- what the device holds
    def _split(self, flat):
        """A flat parameter-shaped vector -> dict in the state dict's names."""
        out, off = {}, 0
        for name, shape in self._shapes:
            size = int(np.prod(shape))
            out[name] = torch.from_numpy(flat[off:off + size].reshape(shape).copy())
            off += size
        assert off == flat.size
        return out

    def _join(self, tensors):
        flat = np.ascontiguousarray(np.concatenate([tensors[name].detach().cpu().numpy().reshape(-1) for name, _ in self._shapes]), dtype=np.float32)
        assert flat.size == self.num_parameters
        return flat

    def step_losses(self):
        """The E * T fp32 step losses of the last `update` (the trainers that run groups of steps)."""
        self._need_handle()
        out = np.empty(self._last_steps, np.float32)
        self._call("step_losses", out.ctypes.data, out.size)
        return torch.from_numpy(out)

    def state_dict(self):
        """The module's state dict: the trained tensors as they stand on the device, every other entry as given."""
        self._need_handle()
        flat = np.empty(self.num_parameters, np.float32)
        self._call("get_parameters", flat.ctypes.data)
        return {**self._split(flat), **{k: v.clone() for k, v in self._rest.items()}}

    def set_untrained(self, name, tensor):
        """Replaces one of the entries `state_dict()` returns as given (a runner's `std`, say); nothing on the device moves."""
        if name not in self._rest:
            raise KeyError(f"{name} is not an untrained entry of the state dict")
        self._rest[name] = tensor.detach().clone()

    def optimizer_state(self):
        """Masters, both Adam moments, the step count and the learning rate."""
        self._need_handle()
        bufs = [np.empty(self.num_parameters, np.float32) for _ in range(3)]
        step, lr = C.c_int64(), C.c_double()
        self._call("get_state", *[b.ctypes.data for b in bufs], C.byref(step), C.byref(lr))
        return dict(parameters=self._split(bufs[0]), exp_avg=self._split(bufs[1]), exp_avg_sq=self._split(bufs[2]), step=step.value, learning_rate=lr.value)

    def load_optimizer_state(self, state):
        self._need_handle()
        bufs = [self._join(state[k]) for k in ("parameters", "exp_avg", "exp_avg_sq")]
        self._call("set_state", *[b.ctypes.data for b in bufs], int(state["step"]), float(state["learning_rate"]))
        self.learning_rate = float(state["learning_rate"])

    def load_state_dict(self, state_dict):
        """New parameters (the trained entries of the module's state dict); the moments, the step count and the learning rate stay."""
        state = self.optimizer_state()
        state["parameters"] = state_dict
        self.load_optimizer_state(state)

    # ---- the carried state (the trainers with `_carry`)
    def get_hidden_states(self, running=False):
        """The state the next update's epochs start from (`last_hidden_states`): `h` (L, N, H) for a GRU, `(h, c)` for an LSTM, None before the
        first update.  `running=True`: the state after the last step run instead (what a loop of `group` calls hands to `set_hidden_states`)."""
        if self.handle is None:
            return None
        N = int(self._fn("get_carry")(self.handle, None, None, 0, 0, self._stream()))
        if N <= 0:
            return None
        L, H, lstm = self._carry
        h = torch.empty(L, N, H, dtype=torch.float32, device=self.device if self._carry_on_device else "cpu")
        c = torch.empty_like(h) if lstm else None
        got = self._fn("get_carry")(self.handle, _ptr(h), _ptr(c), N, 1 if running else 0, self._stream())
        if got != N:
            self._check(int(got), self._prefix + "get_carry")
        return (h.to(self.device), c.to(self.device)) if lstm else h.to(self.device)

    def set_hidden_states(self, hidden_states):
        """Installs the carried state (None: forgets it; the next update starts from zeros, with any number of rows)."""
        self._need_handle()
        if hidden_states is None:
            self._call("reset_carry")
            return
        L, H, _ = self._carry
        parts = hidden_states if isinstance(hidden_states, (tuple, list)) else (hidden_states,)
        parts = [p.detach().to(device=self.device if self._carry_on_device else "cpu", dtype=torch.float32).contiguous() for p in parts]
        N = parts[0].shape[1]
        assert all(tuple(p.shape) == (L, N, H) for p in parts)
        self._ensure(N)
        self._call("set_carry", _ptr(parts[0]), _ptr(parts[1]) if len(parts) > 1 else None, N)

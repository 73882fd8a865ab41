"""`NativeEmpiricalNormalization`: `EmpiricalNormalization` of the vendored rsl_rl (`modules/normalizer.py:14-76`) on the library's normaliser handle
(`lg_obsnorm`, include/lgrunner.h): the running mean / variance / std and the count live on the device, the column moments of a batch are reduced
by one kernel in float64 with a fixed merge order, and `collect_rollout_tracked` runs the same handle between the launches of the one-call
collection.  `state_dict()` has the module's keys, shapes and dtypes: rsl_rl loads what this saves, and this loads what rsl_rl saves."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd.native import load_library
from .policy import _NativeHandle, _ptr


def _runner_lib():
    return load_library("policy", "policy_wide", "runner", "runner_privileged", "runner_distill")


STATE_KEYS = ("_mean", "_var", "_std", "count")


def normalizer_state_dict(mean, var, std, count):
    """The module's `state_dict()` from host arrays: `_mean`, `_var`, `_std` (1, O) float32, `count` an int64 scalar.  No GPU needed."""
    def row(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(1, -1)).copy())
    return {"_mean": row(mean), "_var": row(var), "_std": row(std), "count": torch.tensor(int(count), dtype=torch.long)}


class NativeEmpiricalNormalization(_NativeHandle):
    """Same surface as the module: `__call__` (updates in training mode), `update`, `inverse`, `train` / `eval`, `mean`, `std`, `count`,
    `state_dict` / `load_state_dict`; `forget_carried()` drops the carried row of the tracked collector (include/lgrunner.h)."""
    _destroy = "lg_obsnorm_destroy"

    def __init__(self, shape, eps=1e-2, until=None, device="cuda:0"):
        dims = [int(shape)] if isinstance(shape, int) else [int(s) for s in shape]
        if len(dims) != 1:
            raise NotImplementedError("NativeEmpiricalNormalization normalises rows: shape must be [O]")
        index = self._open(device, "normaliser")
        self.lib = _runner_lib()
        self.num_features, self.eps, self.until = dims[0], float(eps), until
        self.training = True
        self._created(self.lib.lg_obsnorm_create(dims[0], self.eps, -1 if until is None else int(until), index), "lg_obsnorm_create")

    # ---- mode
    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    # ---- the module's calls
    def _rows(self, x):
        x = x.to(device=self.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.num_features:
            raise ValueError(f"expected rows of {self.num_features} values, got {tuple(x.shape)}")
        if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < self.num_features):
            x = x.contiguous()          # (rows of a wider buffer stay as they are: the kernels take the row stride)
        return x, (x.stride(0) if x.shape[0] > 1 else self.num_features)

    def _step(self, x, update, out):
        x, stride = self._rows(x)
        if out == "new":
            out = torch.empty_strided(x.shape, (stride, 1), device=self.device, dtype=torch.float32) if x.shape[0] else torch.empty_like(x)
        elif out == "inplace":
            out = x
        self._check(self.lib.lg_obsnorm_step(self.handle, _ptr(x), x.shape[0], stride, int(update), _ptr(out), self._stream()), "lg_obsnorm_step")
        return out

    def __call__(self, x):
        return self._step(x, self.training, "new")

    forward = __call__

    def normalize_(self, x):
        """`__call__` in place on a float32 tensor of rows on this device (rows may be strided, columns not).  Anything the kernels would have to
        convert first is refused: a converted copy would be normalised and the caller's tensor left raw."""
        here = isinstance(x, torch.Tensor) and x.device.type == "cuda" and (self.device.index is None or x.device.index == self.device.index)
        if not (here and x.dtype == torch.float32 and x.dim() == 2 and
                (x.shape[1] <= 1 or x.stride(1) == 1) and (x.shape[0] <= 1 or x.stride(0) >= self.num_features)):
            raise ValueError("normalize_ works in place: it takes a float32 tensor of rows on the normaliser's device with unit column stride")
        return self._step(x, self.training, "inplace")

    def update(self, x):
        self._step(x, True, None)

    def step_pair(self, other, x, x_other, inplace=False):
        """`self(x)` and `other(x_other)` over the same number of rows in one call (`lg_obsnorm_step_pair`, include/lgrunner_privileged.h): three
        launches for both handles instead of six, the bits of the two single calls.  Both handles must be in the same mode (the runner switches them
        together); each one's `until` freezes its own statistics.  Returns the two normalised tensors; `inplace`: the inputs themselves, under the
        conditions of `normalize_`."""
        if self.training != other.training:
            raise ValueError("step_pair: the two normalisers are in different modes")
        if inplace:
            for norm, t in ((self, x), (other, x_other)):
                if not (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.float32 and t.dim() == 2 and
                        (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= norm.num_features)):
                    raise ValueError("step_pair(inplace=True) takes float32 tensors of rows on the normalisers' device with unit column stride")
        (xa, sa), (xc, sc) = self._rows(x), other._rows(x_other)
        if xa.shape[0] != xc.shape[0]:
            raise ValueError(f"step_pair: {xa.shape[0]} and {xc.shape[0]} rows")
        outs = []
        for t, stride in ((xa, sa), (xc, sc)):
            outs.append(t if inplace else (torch.empty_strided(t.shape, (stride, 1), device=self.device, dtype=torch.float32) if t.shape[0] else torch.empty_like(t)))
        self._check(self.lib.lg_obsnorm_step_pair(self.handle, _ptr(xa), sa, _ptr(outs[0]), other.handle, _ptr(xc), sc, _ptr(outs[1]), xa.shape[0],
                                                  int(self.training), self._stream()), "lg_obsnorm_step_pair")
        return outs[0], outs[1]

    def inverse(self, y):
        y, stride = self._rows(y)
        out = torch.empty_strided(y.shape, (stride, 1), device=self.device, dtype=torch.float32) if y.shape[0] else torch.empty_like(y)
        self._check(self.lib.lg_obsnorm_inverse(self.handle, _ptr(y), y.shape[0], stride, _ptr(out), self._stream()), "lg_obsnorm_inverse")
        return out

    # ---- the carried row of the tracked collector
    def forget_carried(self):
        self._check(self.lib.lg_obsnorm_forget_carried(self.handle), "lg_obsnorm_forget_carried")

    def carried_row(self, n):
        """The (n, O) carried row, or None when the handle holds none of n rows."""
        out = torch.empty(int(n), self.num_features, device=self.device)
        rc = self.lib.lg_obsnorm_carried(self.handle, _ptr(out), int(n), self._stream())
        if rc < 0:
            self._check(rc, "lg_obsnorm_carried")
        return out if rc == 1 else None

    # ---- state
    def get_state(self):
        """Host arrays (mean, var, std) of O float32 and the count."""
        bufs = [np.empty(self.num_features, np.float32) for _ in range(3)]
        count = C.c_int64()
        self._check(self.lib.lg_obsnorm_get_state(self.handle, *[b.ctypes.data for b in bufs], C.byref(count), self._stream()), "lg_obsnorm_get_state")
        return bufs[0], bufs[1], bufs[2], count.value

    def set_state(self, mean, var, std, count):
        bufs = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (mean, var, std)]
        assert all(b.size == self.num_features for b in bufs)
        self._check(self.lib.lg_obsnorm_set_state(self.handle, *[b.ctypes.data for b in bufs], int(count), self._stream()), "lg_obsnorm_set_state")

    def _fetch(self, which):
        """One piece of the state (0 mean, 1 var, 2 std: O float32; 3: the count) in one copy."""
        if which == 3:
            count = C.c_int64()
            self._check(self.lib.lg_obsnorm_get_state(self.handle, None, None, None, C.byref(count), self._stream()), "lg_obsnorm_get_state")
            return count.value
        buf = np.empty(self.num_features, np.float32)
        ptrs = [buf.ctypes.data if k == which else None for k in range(3)]
        self._check(self.lib.lg_obsnorm_get_state(self.handle, *ptrs, None, self._stream()), "lg_obsnorm_get_state")
        return buf

    @property
    def mean(self):
        return torch.from_numpy(self._fetch(0)).to(self.device)

    @property
    def std(self):
        return torch.from_numpy(self._fetch(2)).to(self.device)

    @property
    def count(self):
        return torch.tensor(self._fetch(3), dtype=torch.long, device=self.device)          # (the module's buffer lives on its device)

    def state_dict(self):
        return normalizer_state_dict(*self.get_state())

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in STATE_KEYS if k not in state_dict]
        if missing:
            raise KeyError(f"missing keys in the normaliser's state dict: {missing}")
        self.set_state(*[state_dict[k].detach().cpu().numpy() for k in STATE_KEYS[:3]], int(state_dict["count"]))

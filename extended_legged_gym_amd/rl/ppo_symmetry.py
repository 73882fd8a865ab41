"""`NativeSymmetricPPO`: `NativePPO` with rsl_rl's `symmetry_cfg` (`algorithms/ppo.py:234-370`): symmetric data augmentation and the mirror loss, on
the library's kernels (include/lgtrain_symmetry.h).  The `data_augmentation_func` is probed once on the CPU (`rl/symmetry.py`) and handed to the
library as signed-permutation tables, which the kernels apply while they stage rows: no augmented batch is built and no Python runs inside `update`."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from .policy import _ptr
from .ppo import NativePPO
from .symmetry import resolve_callable, signed_permutation_tables

SYMMETRY_KEYS = ("use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff", "data_augmentation_func", "_env")


class NativeSymmetricPPO(NativePPO):
    """rsl_rl's `PPO` with `symmetry_cfg` for a feed-forward `NativeActorCritic`: the surface of `NativePPO`, and `"symmetry"` in the loss dict.
    `symmetry_cfg`: the reference's keys -- `use_data_augmentation`, `use_mirror_loss`, `mirror_loss_coeff`, `data_augmentation_func` (a callable or
    `"module:function"`), `_env` (passed to the function while it is probed)."""
    _destroy = "lg_ppo_sym_destroy"
    _prefix = "lg_ppo_sym_"
    _unit = "train_symmetry"

    def __init__(self, policy, state_dict, symmetry_cfg=None, **kw):
        if not symmetry_cfg:
            raise ValueError("NativeSymmetricPPO needs a symmetry_cfg; NativePPO is the trainer without one")
        for name in ("actor", "critic"):          # the symmetric forward stages a whole mirrored row at once: no split-K first layer there
            width = getattr(policy, name).dims[0] if hasattr(policy, name) else 0
            if width > abi.MLP_MAX_WIDTH:
                raise NotImplementedError(f"NativeSymmetricPPO: the {name} reads rows of {width} columns; the symmetric update takes at most "
                                          f"{abi.MLP_MAX_WIDTH} (NativePPO trains wide rows, without the symmetry terms)")
        unknown = set(symmetry_cfg) - set(SYMMETRY_KEYS)
        if unknown:
            raise ValueError(f"symmetry_cfg: unknown keys {sorted(unknown)} (known: {', '.join(SYMMETRY_KEYS)})")
        self.use_data_augmentation = bool(symmetry_cfg.get("use_data_augmentation", False))
        self.use_mirror_loss = bool(symmetry_cfg.get("use_mirror_loss", False))
        self.mirror_loss_coeff = float(symmetry_cfg.get("mirror_loss_coeff", 0.0))
        func = resolve_callable(symmetry_cfg.get("data_augmentation_func"))
        if not callable(func):
            raise ValueError(f"symmetry_cfg: data_augmentation_func is not callable: {func}")
        self.data_augmentation_func, env = func, symmetry_cfg.get("_env")
        self._tables = None
        max_rows = kw.pop("max_rows", None)
        super().__init__(policy, state_dict, max_rows=None, **kw)          # refuses the options NativePPO refuses, recurrent policies among them
        O, Oc, A = policy.actor.dims[0], policy.critic.dims[0], policy.num_actions
        self._tables = (signed_permutation_tables(func, O, "observations", "policy", env), signed_permutation_tables(func, Oc, "observations", "critic", env),
                        signed_permutation_tables(func, A, "actions", "policy", env))
        blocks = {t[0].shape[0] for t in self._tables}
        if len(blocks) != 1:
            raise ValueError(f"data_augmentation_func returns {[t[0].shape[0] for t in self._tables]} blocks for policy observations, critic "
                             "observations and actions: they must agree")
        self.num_blocks = blocks.pop()
        self._stats = torch.zeros(6, dtype=torch.float64, device=self.device)
        if max_rows is not None:
            self._create(int(max_rows))

    # ---- handle
    def _make_handle(self, max_rows, tables=None):
        fp = C.POINTER(C.c_float)

        def lists(layers):
            return ((fp * len(layers))(*[w.ctypes.data_as(fp) for w, _ in layers]), (fp * len(layers))(*[b.ctypes.data_as(fp) for _, b in layers]))
        aw, ab = lists(self._alayers)
        cw, cb = lists(self._clayers)
        (op, os_), (cp, cs), (ap, as_) = [(np.ascontiguousarray(p, np.int32), np.ascontiguousarray(s, np.float32)) for p, s in (tables or self._tables)]
        tab = abi.lg_ppo_sym_tables(op.shape[0], op.shape[1], cp.shape[1], ap.shape[1], op.ctypes.data, os_.ctypes.data, cp.ctypes.data, cs.ctypes.data,
                                    ap.ctypes.data, as_.ctypes.data)
        cfg = abi.lg_ppo_sym_config(int(self.use_data_augmentation), int(self.use_mirror_loss), self.mirror_loss_coeff)
        return self._fn("create")(self.policy.actor.handle, self.policy.critic.handle, aw, ab, cw, cb, self._std0.ctypes.data,
                                  abi.NOISE_STD_TYPES[self.policy.noise_std_type], self.learning_rate, max_rows, _ptr(self.policy.std), C.byref(tab), C.byref(cfg))

    # ---- training
    def update(self, rollout, indices=None):
        """`NativePPO.update`; the loss dict also carries `"symmetry"`, the mean symmetry loss over the optimiser steps (ppo.py:409-436)."""
        loss = super().update(rollout, indices)
        loss["symmetry"] = self._last_stats[5]
        return loss

    # ---- what the device holds
    def gradients(self):
        """As `NativePPO.gradients`; the means also carry the mini-batch's `"symmetry"` loss."""
        self._need_handle()
        g, norm, means, sym = np.empty(self.num_parameters, np.float32), C.c_float(), (C.c_float * 4)(), C.c_float()
        self._call("gradients", g.ctypes.data, C.byref(norm), means, C.byref(sym))
        out = dict(zip(("surrogate", "value_function", "entropy", "kl"), [float(x) for x in means]))
        out["symmetry"] = float(sym.value)
        return self._split(g), norm.value, out

    def forward_outputs(self, count):
        """The last mini-batch's action means (num_blocks * count, A), block k of mini-batch row j at k * count + j, and values: (num_blocks * count, 1)
        with data augmentation, (count, 1) without -- the critic does not see transformed rows then."""
        self._need_handle()
        K = self.num_blocks
        mu = np.empty((K * count, self.policy.num_actions), np.float32)
        val = np.empty(((K if self.use_data_augmentation else 1) * count, 1), np.float32)
        self._call("forward_outputs", mu.ctypes.data, val.ctypes.data)
        return torch.from_numpy(mu), torch.from_numpy(val)

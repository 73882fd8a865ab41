"""`NativeRecurrentPPO`: `PPO.update` of the vendored rsl_rl for a `NativeActorCriticRecurrent` (`algorithms/ppo.py:197-438` with the mini-batches of
`storage/rollout_storage.py:246-316`: env slices over all T steps, the same slices every epoch, no permutation), on the library's recurrent training
kernels (include/lgtrain_recurrent.h): backpropagation through time through the LSTM / GRU memories without the reference's padding -- a row enters
step t with the hidden row saved at t when t == 0 or the env was done at t - 1, else with its own state after t - 1.  The weights stay on the device
and are updated in place, in the tiled images `policy.act*` and `collect_rollout` read."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from .policy import NativeActorCriticRecurrent, _ptr
from .ppo import NativePPO, _sequential_layers

RNN_TENSORS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


class NativeRecurrentPPO(NativePPO):
    """rsl_rl's `PPO` for a `NativeActorCriticRecurrent`, with its names and defaults and the surface of `NativePPO`.  `state_dict`: the
    `ActorCriticRecurrent` state dict `policy` was built from (`memory_a.rnn.*`, `memory_c.rnn.*`, `actor.*`, `critic.*`, `std` / `log_std`); it seeds
    the fp32 masters.  After `update`, the same `policy` object acts with the new weights; nothing is rebuilt."""
    _destroy = "lg_ppo_recurrent_destroy"
    _prefix = "lg_ppo_recurrent_"
    _unit = "train_recurrent"

    def __init__(self, policy, state_dict, num_learning_epochs=5, num_mini_batches=4, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.0,
                 learning_rate=1e-3, schedule="fixed", desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True, max_rows=None,
                 normalize_advantage_per_mini_batch=False, rnd_cfg=None, symmetry_cfg=None, multi_gpu_cfg=None):
        if not isinstance(policy, NativeActorCriticRecurrent):
            raise TypeError("NativeRecurrentPPO trains a NativeActorCriticRecurrent")
        for name, value in (("normalize_advantage_per_mini_batch", normalize_advantage_per_mini_batch), ("rnd_cfg", rnd_cfg),
                            ("symmetry_cfg", symmetry_cfg), ("multi_gpu_cfg", multi_gpu_cfg)):
            if value:
                raise NotImplementedError(f"{name} is not built in the native update")
        if schedule not in abi.LR_SCHEDULES:
            raise ValueError(f"Unknown schedule: {schedule}. Should be 'fixed' or 'adaptive'")
        self._open_trainer(policy.device)
        self.policy = policy
        self.num_learning_epochs, self.num_mini_batches = int(num_learning_epochs), int(num_mini_batches)
        self.clip_param, self.value_loss_coef, self.entropy_coef = float(clip_param), float(value_loss_coef), float(entropy_coef)
        self.schedule, self.desired_kl, self.max_grad_norm = schedule, float(desired_kl if desired_kl is not None else 0.0), float(max_grad_norm)
        self.use_clipped_value_loss = bool(use_clipped_value_loss)
        self.learning_rate = float(learning_rate)
        self.max_rows = max_rows
        self.std_key = "std" if policy.noise_std_type == "scalar" else "log_std"
        self._aidx, self._alayers = _sequential_layers(state_dict, "actor")
        self._cidx, self._clayers = _sequential_layers(state_dict, "critic")
        self._std0 = np.ascontiguousarray(state_dict[self.std_key].detach().cpu().numpy(), dtype=np.float32)
        G = 4 if policy.memory_a.rnn_type == "lstm" else 3
        self._mem = {}
        for prefix, mem in (("memory_a", policy.memory_a), ("memory_c", policy.memory_c)):
            L = len([k for k in state_dict if k.startswith(prefix + ".rnn.weight_ih_l")])
            arrs = [[np.ascontiguousarray(state_dict[f"{prefix}.rnn.{name}_l{l}"].detach().cpu().numpy(), dtype=np.float32) for name in RNN_TENSORS]
                    for l in range(L)]
            if L != mem.num_layers or arrs[0][0].shape != (G * mem.hidden_size, mem.input_size) or arrs[0][1].shape != (G * mem.hidden_size, mem.hidden_size):
                raise ValueError(f"{prefix}.rnn.* of the state dict does not have the shapes of the policy's {mem.rnn_type} memory "
                                 f"({mem.num_layers} layers, {mem.input_size} -> {mem.hidden_size})")
            self._mem[prefix] = arrs
        # the flat order of include/lgtrain_recurrent.h: actor, critic, memory_a, memory_c (per layer weight_ih, weight_hh, bias_ih, bias_hh), std
        self._shapes = []
        for prefix, idx, layers in (("actor", self._aidx, self._alayers), ("critic", self._cidx, self._clayers)):
            for i, (w, b) in zip(idx, layers):
                self._shapes += [(f"{prefix}.{i}.weight", w.shape), (f"{prefix}.{i}.bias", b.shape)]
        for prefix in ("memory_a", "memory_c"):
            for l, arr in enumerate(self._mem[prefix]):
                self._shapes += [(f"{prefix}.rnn.{name}_l{l}", a.shape) for name, a in zip(RNN_TENSORS, arr)]
        self._shapes.append((self.std_key, self._std0.shape))
        self._stats = torch.zeros(5, dtype=torch.float64, device=self.device)
        if max_rows is not None:
            self._create(int(max_rows))

    # ---- handle
    def _make_handle(self, max_rows):
        fp = C.POINTER(C.c_float)

        def plist(arrays):
            return (fp * len(arrays))(*[a.ctypes.data_as(fp) for a in arrays])
        pol = self.policy
        lists = {}
        for tag, prefix in (("mem_a", "memory_a"), ("mem_c", "memory_c")):
            for j, name in enumerate(("w_ih", "w_hh", "b_ih", "b_hh")):
                lists[f"{tag}_{name}"] = plist([layer[j] for layer in self._mem[prefix]])
        lists.update(actor_weights=plist([w for w, _ in self._alayers]), actor_biases=plist([b for _, b in self._alayers]),
                     critic_weights=plist([w for w, _ in self._clayers]), critic_biases=plist([b for _, b in self._clayers]))
        params = abi.lg_ppo_recurrent_params(rnn_type=abi.RNN_TYPES[pol.memory_a.rnn_type], num_layers=len(self._mem["memory_a"]),
                                             input_a=self._mem["memory_a"][0][0].shape[1], hidden_a=self._mem["memory_a"][0][1].shape[1],
                                             input_c=self._mem["memory_c"][0][0].shape[1], hidden_c=self._mem["memory_c"][0][1].shape[1],
                                             std=self._std0.ctypes.data, **lists)
        return self._fn("create")(pol.memory_a.handle, pol.actor.handle, pol.memory_c.handle, pol.critic.handle, C.byref(params),
                                  abi.NOISE_STD_TYPES[pol.noise_std_type], self.learning_rate, max_rows, _ptr(pol.std))

    def _rollout(self, rollout):
        """The (T, N, .) tensors of a recurrent `collect_rollout` dict as the library takes them, kept alive by the returned list."""
        for key in ("dones", "hidden_states_a", "hidden_states_c"):
            if key not in rollout:
                raise KeyError(f"the rollout has no {key}: a recurrent update needs the dones and the hidden-state rows collect_rollout keeps")

        def f32(t):
            return t.to(device=self.device, dtype=torch.float32).contiguous()

        def get(*keys):
            return f32(rollout[next(k for k in keys if k in rollout)])
        keep = dict(observations=get("observations"), critic_observations=get("critic_observations", "privileged_observations", "observations"),
                    actions=get("actions"), values=get("values"), returns=get("returns"), advantages=get("advantages"),
                    actions_log_prob=get("actions_log_prob"), mu=get("mu"), sigma=get("sigma"))
        pol = self.policy
        T, N = keep["observations"].shape[:2]
        assert keep["observations"].shape == (T, N, pol.memory_a.input_size) and keep["critic_observations"].shape == (T, N, pol.memory_c.input_size)
        assert keep["actions"].shape == (T, N, pol.num_actions)
        dones = f32(rollout["dones"]).reshape(T, N)
        hid = []
        for key, mem in (("hidden_states_a", pol.memory_a), ("hidden_states_c", pol.memory_c)):
            hs = rollout[key]
            parts = [f32(x) for x in (hs if isinstance(hs, (tuple, list)) else (hs,))]
            if len(parts) != (2 if mem.rnn_type == "lstm" else 1):
                raise ValueError(f"{key}: an lstm keeps (h, c), a gru keeps h")
            for x in parts:
                assert x.shape == (T, mem.num_layers, N, mem.hidden_size), (key, tuple(x.shape))
            hid.append(parts + [None] * (2 - len(parts)))
        hidden = abi.lg_rollout_hidden(h_a=hid[0][0].data_ptr(), c_a=hid[0][1].data_ptr() if hid[0][1] is not None else None,
                                       h_c=hid[1][0].data_ptr(), c_c=hid[1][1].data_ptr() if hid[1][1] is not None else None)
        return abi.lg_ppo_rows(**{k: v.data_ptr() for k, v in keep.items()}), hidden, dones, T, N, [keep, hid]

    # ---- training
    def minibatch(self, rollout, env0, count):
        """One optimiser step on the env slice [env0, env0 + count) over all T steps; mini-batch row t * count + j is env env0 + j at step t."""
        rows, hidden, dones, T, N, keep = self._rollout(rollout)
        self._ensure(T * int(count))
        hyper = self._hyper()
        self._call("minibatch", C.byref(rows), C.byref(hidden), _ptr(dones), T, N, int(env0), int(count), C.byref(hyper))
        del keep

    def update(self, rollout):
        """`PPO.update` on the dict `collect_rollout` returns for a recurrent policy: `num_learning_epochs` passes over the `num_mini_batches` env slices
        of `N // num_mini_batches` envs.  Returns the loss dict of `PPO.update`; `learning_rate` and `kl` are refreshed by the one copy at the end."""
        rows, hidden, dones, T, N, keep = self._rollout(rollout)
        self._ensure(T * max(N // self.num_mini_batches, 1))
        hyper = self._hyper()
        self._call("update", C.byref(rows), C.byref(hidden), _ptr(dones), T, N, self.num_mini_batches, self.num_learning_epochs, C.byref(hyper), _ptr(self._stats))
        st = self._stats.cpu().tolist()
        del keep
        self.learning_rate, self.kl = st[4], st[3]
        return {"value_function": st[0], "surrogate": st[1], "entropy": st[2]}

    # ---- what the device holds
    def images(self, memory, layer):
        """The device images of one memory layer as the acts read them: (tiled weights, tiled bias), float32 numpy."""
        self._need_handle()
        mem = self.policy.memory_a if memory == 0 else self.policy.memory_c
        G, H = (4 if mem.rnn_type == "lstm" else 3), mem.hidden_size
        if layer == 0 and mem.input_size > abi.RNN_MAX_WIDTH:          # a wide memory: the seeded step's image (weight_hh alone; lgpolicy_wide_memory.h)
            size = C.c_int64(0)
            self.lib.lg_rnn_tile_weights_wide(abi.RNN_TYPES[mem.rnn_type], mem.input_size, H, None, None, None, None, C.byref(size))
            count = size.value
        else:
            count = int(self.lib.lg_rnn_tile_weights(abi.RNN_TYPES[mem.rnn_type], mem.input_size if layer == 0 else H, H, None, None, None))
        w, b = np.empty(count, np.float32), np.empty(4 * 16 * ((H + 15) // 16), np.float32)
        self._call("get_images", memory, layer, w.ctypes.data, b.ctypes.data)
        return w, b

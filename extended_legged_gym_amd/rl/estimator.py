"""`NativeTerrainEstimator`: the reference's `TerrainEstimator` (`rsl_rl/modules/terrain_estimator.py:13-218`: depth-image CNN encoder ->
combination layer with the base velocities -> GRU / LSTM `Memory` -> MLP decoder, predicting the ray caster's distances) in inference mode on
`lg_conv_encoder_forward` / `lg_estimator_step` (include/lgpolicy.h).  The weights come from a checkpoint of the reference's module, by its own
key names; gradients (`EstimatorDistillation.update`) are `rl.NativeEstimatorDistillation` (`rl/estimator_distillation.py`), which trains this
object's weights in place, or eager PyTorch (`tools/train_estimator.py --update torch`)."""
import ctypes as C

import numpy as np
import torch

from extended_legged_gym_amd import abi
from .policy import NativeMemory, NativeMLP, _NativeHandle, _ptr

ENCODER_KEYS = (0, 2, 4, 6, 10, 12)                      # Conv2d x 4, Linear x 2 of depth_encoder (terrain_estimator.py:85-107)
_CONV_SHAPES = ((32, 1, 5, 5), (64, 32, 3, 3), (128, 64, 3, 3), (64, 128, 3, 3))


def estimator_activation(name):
    """`elu | relu | tanh`; anything else falls back to ELU, as the module does (`terrain_estimator.py:44-51`)."""
    name = str(name).lower()
    return name if name in ("elu", "relu", "tanh") else "elu"


def parse_precision(name):
    """`fp32 | bf16` -> LG_PREC_*; ValueError for anything else (no device needed)."""
    if not isinstance(name, str) or name not in abi.ENCODER_PRECISIONS:
        raise ValueError(f"encoder precision {name!r}: must be one of {sorted(abi.ENCODER_PRECISIONS)}")
    return abi.ENCODER_PRECISIONS[name]


def parse_estimator_state(state_dict, depth_image_shape, proprio_dim, memory_type="gru"):
    """The loading rules of `NativeTerrainEstimator`, without a device.  `state_dict`: a `TerrainEstimator.state_dict()`, or a runner file's
    dict holding one under `model_state_dict` (`terrain_estimator_runner.py:568-578`).  Returns a dict: `encoder` [(weight, bias)] x 6,
    `combine` (weight, bias), `memory` [(w_ih, w_hh, b_ih, b_hh)] per layer, `decoder` [(weight, bias)], and the widths read from the shapes
    (`encoder_output_dim`, `memory_hidden_size`, `memory_num_layers`, `decoder_hidden_dims`, `num_raycast_outputs`).  ValueError naming the
    key whose shape does not fit the declared image, `proprio_dim` or memory type, or the width of a combination layer wider than an `lg_mlp`
    takes; KeyError for a missing key."""
    if "model_state_dict" in state_dict and "depth_encoder.0.weight" not in state_dict:
        state_dict = state_dict["model_state_dict"]
    height, width = (int(v) for v in depth_image_shape)
    if not (abi.ENCODER_MIN_SIDE <= height <= abi.ENCODER_MAX_SIDE and abi.ENCODER_MIN_SIDE <= width <= abi.ENCODER_MAX_SIDE):
        raise ValueError(f"depth_image_shape {(height, width)}: each side must be in {abi.ENCODER_MIN_SIDE}..{abi.ENCODER_MAX_SIDE}")
    memory_type = str(memory_type).lower()
    if memory_type not in abi.RNN_TYPES:
        raise ValueError(f"Unknown memory_type: {memory_type}. Should be 'lstm' or 'gru'")

    def arr(key):
        if key not in state_dict:
            raise KeyError(f"{key} is not in the state dict: not a TerrainEstimator checkpoint")
        v = state_dict[key]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        return np.ascontiguousarray(v, dtype=np.float32)

    def pair(prefix, shape, why):
        w, b = arr(prefix + ".weight"), arr(prefix + ".bias")
        if shape is not None and w.shape != tuple(shape):
            raise ValueError(f"{prefix}.weight has shape {w.shape}, expected {tuple(shape)} ({why})")
        if b.shape != (w.shape[0],):
            raise ValueError(f"{prefix}.bias has shape {b.shape}, expected {(w.shape[0],)}")
        return w, b

    enc = [pair(f"depth_encoder.{i}", s, "the fixed topology of the depth encoder") for i, s in zip(ENCODER_KEYS[:4], _CONV_SHAPES)]
    enc.append(pair("depth_encoder.10", (128, 64 * 4 * 4), "Linear after AdaptiveAvgPool2d((4, 4)) of 64 channels"))
    w12 = arr("depth_encoder.12.weight")
    if w12.ndim != 2 or w12.shape[1] != 128 or not 1 <= w12.shape[0] <= abi.ENCODER_MAX_OUT:
        raise ValueError(f"depth_encoder.12.weight has shape {w12.shape}, expected (encoder_output_dim <= {abi.ENCODER_MAX_OUT}, 128)")
    enc.append(pair("depth_encoder.12", None, ""))
    F = w12.shape[0]
    if F + int(proprio_dim) > abi.MLP_MAX_WIDTH:
        raise ValueError(f"the combination layer reads encoder_output_dim {F} + proprio_dim {int(proprio_dim)} = {F + int(proprio_dim)} inputs, more than the "
                         f"{abi.MLP_MAX_WIDTH} an lg_mlp layer takes")
    comb = pair("combination_mlp.0", (F, F + int(proprio_dim)), f"encoder_output_dim {F} + proprio_dim {int(proprio_dim)} inputs")
    G = 4 if memory_type == "lstm" else 3
    L = len([k for k in state_dict if k.startswith("memory.rnn.weight_ih_l")])
    if L == 0:
        raise KeyError("memory.rnn.weight_ih_l0 is not in the state dict: not a TerrainEstimator checkpoint")
    whh = arr("memory.rnn.weight_hh_l0")
    if whh.ndim != 2 or whh.shape[0] != G * whh.shape[1]:
        raise ValueError(f"memory.rnn.weight_hh_l0 has shape {whh.shape}: not the ({G} H, H) of an nn.{memory_type.upper()}")
    H = whh.shape[1]
    mem = []
    for l in range(L):
        layer = [arr(f"memory.rnn.{name}_l{l}") for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        want = ((G * H, F if l == 0 else H), (G * H, H), (G * H,), (G * H,))
        for name, a, s in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), layer, want):
            if a.shape != s:
                raise ValueError(f"memory.rnn.{name}_l{l} has shape {a.shape}, expected {s} (nn.{memory_type.upper()} of hidden size {H} on {F} inputs)")
        mem.append(tuple(layer))
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith("decoder.") and k.endswith(".weight")})
    if not idx:
        raise KeyError("decoder.0.weight is not in the state dict: not a TerrainEstimator checkpoint")
    dec, cur = [], H
    for i in idx:
        w = arr(f"decoder.{i}.weight")
        if w.ndim != 2 or w.shape[1] != cur:
            raise ValueError(f"decoder.{i}.weight has shape {w.shape}, expected (*, {cur})")
        dec.append(pair(f"decoder.{i}", None, ""))
        cur = w.shape[0]
    return dict(encoder=enc, combine=comb, memory=mem, decoder=dec, depth_image_shape=(height, width), proprio_dim=int(proprio_dim),
                encoder_output_dim=F, memory_type=memory_type, memory_hidden_size=H, memory_num_layers=L,
                decoder_hidden_dims=[w.shape[0] for w, _ in dec[:-1]], num_raycast_outputs=cur)


class NativeConvEncoder(_NativeHandle):
    """`TerrainEstimator.depth_encoder` (`terrain_estimator.py:80-109`) on the GPU: `layers` = [(weight, bias)] x 6 in torch's layouts.
    `precision`: "fp32" (default), or "bf16" for inference on the bf16 matrix cores (bf16 operands and maps, fp32 accumulation and features;
    include/lgpolicy.h `lg_conv_encoder_create_precision`)."""
    _destroy = "lg_conv_encoder_destroy"

    def __init__(self, layers, depth_image_shape, activation="elu", device="cuda:0", precision="fp32"):
        prec = parse_precision(precision)
        self.precision = precision
        index = self._open(device, "estimator")
        self.height, self.width = (int(v) for v in depth_image_shape)
        ws = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w, _ in layers]
        bs = [np.ascontiguousarray(np.asarray(b, dtype=np.float32)) for _, b in layers]
        self.out_dim = int(ws[5].shape[0])
        fp = C.POINTER(C.c_float)
        wp = (fp * 6)(*[w.ctypes.data_as(fp) for w in ws])
        bp = (fp * 6)(*[b.ctypes.data_as(fp) for b in bs])
        if prec == abi.LG_PREC_F32:
            handle = self.lib.lg_conv_encoder_create(self.height, self.width, self.out_dim, abi.ACTIVATIONS[estimator_activation(activation)], wp, bp, index)
        else:
            handle = self.lib.lg_conv_encoder_create_precision(self.height, self.width, self.out_dim, abi.ACTIVATIONS[estimator_activation(activation)], wp, bp,
                                                               index, prec)
        self._created(handle, "lg_conv_encoder_create")

    def latest_frame(self, depth_images):
        """(n, h, w), or the camera's (n, buffer_len, h, w) FIFO of which the latest frame `[:, -1]` is taken as a view: no copy when the
        images themselves are contiguous."""
        x = depth_images
        if x.dim() == 4:
            x = x[:, -1]
        if x.dim() != 3 or x.shape[1:] != (self.height, self.width):
            raise ValueError(f"depth images of shape {tuple(depth_images.shape)} do not fit the encoder's {(self.height, self.width)}")
        if x.device != self.device or x.dtype != torch.float32:
            x = x.to(device=self.device, dtype=torch.float32)
        if x.stride(2) != 1 or x.stride(1) != self.width or (x.shape[0] > 1 and x.stride(0) < self.height * self.width):
            x = x.contiguous()
        return x

    def __call__(self, depth_images):
        x = self.latest_frame(depth_images)
        n = x.shape[0]
        y = torch.empty(n, self.out_dim, device=self.device)
        self._check(self.lib.lg_conv_encoder_forward(self.handle, _ptr(x), max(x.stride(0), self.height * self.width), n, _ptr(y), self._stream()),
                    "lg_conv_encoder_forward")
        return y

    def stage_shape(self, k):
        """(floats of one row, (H, W, C)) of stage k's output: k = 1..4 the convolutions, 5 pool + flatten, 6 and 7 the linear layers."""
        h, w, c = C.c_int32(), C.c_int32(), C.c_int32()
        count = self.lib.lg_conv_encoder_stage_shape(self.handle, int(k), C.byref(h), C.byref(w), C.byref(c))
        if count < 0:
            raise ValueError("lg_conv_encoder_stage_shape failed: " + (self.lib.lg_mlp_last_error(None) or b"").decode())
        return int(count), (h.value, w.value, c.value)

    def stage(self, depth_images, k, out=None):
        """The encoder cut after stage k (`lg_conv_encoder_forward_stages`): torch's (n, C, H, W) view of a convolution's map (the kernels keep it
        channel last), (n, 1024) after pool + flatten, (n, 128), (n, out_dim).  `out`: a flat float32 buffer of at least n x count floats to
        write into instead of a fresh one."""
        x = self.latest_frame(depth_images)
        n = x.shape[0]
        count, (h, w, c) = self.stage_shape(k)
        if out is None:
            out = torch.empty(n * count, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.device == self.device and out.numel() >= n * count
        self._check(self.lib.lg_conv_encoder_forward_stages(self.handle, _ptr(x), max(x.stride(0), self.height * self.width), n, int(k), _ptr(out), self._stream()),
                    "lg_conv_encoder_forward_stages")
        y = out.view(-1)[:n * count]
        return y.view(n, h, w, c).permute(0, 3, 1, 2) if k <= 4 else y.view(n, count)


class NativeTerrainEstimator:
    """Same surface as `TerrainEstimator` for inference (`terrain_estimator.py:200-218`): `act_inference`, `reset`, `get_hidden_states`,
    `set_hidden_states`.  `encoder_output_dim`, the memory's width / depth and the decoder's widths are read from the checkpoint's shapes.
    `encoder_precision`: "fp32" (default) or "bf16", the mode of the depth encoder alone; combination layer, memory and decoder stay fp32."""

    def __init__(self, state_dict, depth_image_shape, proprio_dim, activation="elu", memory_type="gru", device="cuda:0", encoder_precision="fp32"):
        parse_precision(encoder_precision)          # refused before anything is parsed or built
        self.precision = encoder_precision
        spec = parse_estimator_state(state_dict, depth_image_shape, proprio_dim, memory_type)
        self.spec = {k: v for k, v in spec.items() if k not in ("encoder", "combine", "memory", "decoder")}
        self.device = torch.device(device)
        act = estimator_activation(activation)
        self.depth_image_shape, self.proprio_dim = spec["depth_image_shape"], spec["proprio_dim"]
        self.num_raycast_outputs = spec["num_raycast_outputs"]
        self.encoder = NativeConvEncoder(spec["encoder"], self.depth_image_shape, act, device, precision=encoder_precision)
        self.combine = NativeMLP([spec["combine"]], act, device)
        self.combine._check(self.combine.lib.lg_mlp_set_output_activation(self.combine.handle, 1), "lg_mlp_set_output_activation")
        self.memory = NativeMemory(spec["memory"], spec["memory_type"], device)
        self.decoder = NativeMLP(spec["decoder"], act, device)

    def act_inference(self, depth_images, proprio_data):
        """`TerrainEstimator.act_inference` (`:200-202`): one step for every row, advancing the memory."""
        return self._step(depth_images, proprio_data, None)

    forward = act_inference

    def _step(self, depth_images, proprio_data, reset):
        enc, lib = self.encoder, self.encoder.lib
        x = enc.latest_frame(depth_images)
        n = x.shape[0]
        p = proprio_data.to(device=self.device, dtype=torch.float32).contiguous()
        if p.shape != (n, self.proprio_dim):
            raise ValueError(f"proprio_data of shape {tuple(p.shape)}, expected {(n, self.proprio_dim)}")
        self.memory.ensure_state(n)
        if reset is not None:
            reset = reset.to(device=self.device, dtype=torch.float32).contiguous().view(-1)
            assert reset.shape[0] == n
        out = torch.empty(n, self.num_raycast_outputs, device=self.device)
        enc._check(lib.lg_estimator_step(enc.handle, self.combine.handle, self.memory.handle, self.decoder.handle, _ptr(x), max(x.stride(0), enc.height * enc.width),
                                         _ptr(p), n, *self.memory._ptrs(), _ptr(reset), _ptr(out), enc._stream()), "lg_estimator_step")
        return out

    def reset(self, dones=None, hidden_states=None):
        """`Memory.reset` (`networks/memory.py:35-51`): no arguments forgets the state, `hidden_states` alone installs it, `dones` zeroes those rows."""
        if dones is None:
            if hidden_states is None:
                self.memory.reset(None)
            else:
                self.set_hidden_states(hidden_states)
        else:
            self.memory.reset(dones)

    def get_hidden_states(self):
        return self.memory.hidden_states

    def set_hidden_states(self, hidden_states):
        """`h` (L, n, H) for a GRU, `(h, c)` for an LSTM, None to forget; copied into the live state."""
        self.memory.set_state(hidden_states)

    def close(self):
        for part in (self.encoder, self.combine, self.memory, self.decoder):
            part.close()

"""`TerrainEstimatorTorch`: an own torch restatement of `rsl_rl/modules/terrain_estimator.py:13-218` with the SAME parameter names
(`depth_encoder.{0,2,4,6,10,12}`, `combination_mlp.0`, `memory.rnn`, `decoder.{0,2,..}`), so checkpoints interchange with the reference's module
and with `NativeTerrainEstimator`.  `tests/test_estimator_golden.py` pins it to outputs recorded from the reference's module.  It seeds the native
estimator of `rl.NativeTerrainEstimatorRunner` and is the eager-PyTorch side of `tools/train_estimator.py`."""
import torch
import torch.nn as nn


def _activation(name):
    name = str(name).lower()
    return {"elu": nn.ELU, "relu": nn.ReLU, "tanh": nn.Tanh}.get(name, nn.ELU)()          # anything else: ELU (terrain_estimator.py:44-51)


class _Memory(nn.Module):
    """`rsl_rl/networks/memory.py:14-66` in inference / distillation mode: the state of the last step is kept on the module."""

    def __init__(self, input_size, type="gru", num_layers=1, hidden_size=256):
        super().__init__()
        self.rnn = (nn.GRU if type.lower() == "gru" else nn.LSTM)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None

    def forward(self, x):
        out, self.hidden_states = self.rnn(x.unsqueeze(0), self.hidden_states)
        return out.squeeze(0)

    def _each(self):
        hs = self.hidden_states
        return () if hs is None else (hs if isinstance(hs, tuple) else (hs,))

    def reset(self, dones=None, hidden_states=None):
        if dones is None:
            self.hidden_states = hidden_states
        else:
            for h in self._each():
                h[..., dones == 1, :] = 0.0

    def detach_hidden_states(self):
        if self.hidden_states is not None:
            hs = tuple(h.detach() for h in self._each())
            self.hidden_states = hs if isinstance(self.hidden_states, tuple) else hs[0]


class TerrainEstimatorTorch(nn.Module):
    def __init__(self, depth_image_shape, proprio_dim, num_raycast_outputs, encoder_output_dim=64, memory_hidden_size=256, memory_num_layers=1,
                 memory_type="gru", decoder_hidden_dims=(128, 64), activation="elu"):
        super().__init__()
        self.depth_image_shape, self.proprio_dim, self.num_raycast_outputs = tuple(depth_image_shape), proprio_dim, num_raycast_outputs
        act = _activation(activation)                       # one shared instance, as in the reference: the parameter-free layers take no state-dict keys
        self.depth_encoder = nn.Sequential(
            nn.Conv2d(1, 32, kernel_size=5, stride=2, padding=2), act, nn.Conv2d(32, 64, kernel_size=3, stride=2, padding=1), act,
            nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1), act, nn.Conv2d(128, 64, kernel_size=3, stride=1, padding=1), act,
            nn.AdaptiveAvgPool2d((4, 4)), nn.Flatten(), nn.Linear(64 * 4 * 4, 128), act, nn.Linear(128, encoder_output_dim), act)
        self.combination_mlp = nn.Sequential(nn.Linear(encoder_output_dim + proprio_dim, encoder_output_dim), act)
        self.memory = _Memory(encoder_output_dim, memory_type, memory_num_layers, memory_hidden_size)
        layers, cur = [], memory_hidden_size
        for width in decoder_hidden_dims:
            layers += [nn.Linear(cur, width), act]
            cur = width
        layers.append(nn.Linear(cur, num_raycast_outputs))
        self.decoder = nn.Sequential(*layers)

    def encode(self, depth_images):
        if depth_images.dim() == 4 and depth_images.shape[1] != 1:
            depth_images = depth_images[:, -1]
        if depth_images.dim() == 3:
            depth_images = depth_images.unsqueeze(1)
        return self.depth_encoder(depth_images)

    def forward(self, depth_images, proprio_data):
        x = self.combination_mlp(torch.cat([self.encode(depth_images), proprio_data], dim=-1))
        return self.decoder(self.memory(x))

    act_inference = forward

    def reset(self, dones=None, hidden_states=None):
        self.memory.reset(dones, hidden_states)

    def detach_hidden_states(self):
        self.memory.detach_hidden_states()

    def get_hidden_states(self):
        return self.memory.hidden_states

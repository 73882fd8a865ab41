"""GPU: the terrain estimator on the native side (include/lgpolicy.h `lg_conv_encoder_forward`, `lg_estimator_step`; `NativeConvEncoder`,
`NativeTerrainEstimator`, `collect_estimation`) against float64 torch, the golden vectors recorded from the reference's `TerrainEstimator`, and
the Python collection loop bit for bit.

Tolerance: the rule of tests/test_hip_distillation.py, not a new number -- a bar is max(2e-5, 4 x the gap between torch fp32 and torch float64
on the same case): the gap recorded in the golden file for the golden cases, computed here for the full-size ones.  Each test prints error,
gap and bar."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from extended_legged_gym_amd import abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
G = np.load(os.path.join(ROOT, "tests", "golden", "terrain_estimator.npz"))
FLOOR = 2e-5
T, N, P, R = 6, 8, 6, 81
ENV_OVER = {"terrain.num_rows": 2, "terrain.num_cols": 3, "terrain.confined_terrain_proportions": [0.0, 0.2, 0.4, 0.4]}


def check(tag, got, want64, want32):
    got, want64 = got.detach().double().cpu(), want64.detach().double().cpu()
    gap = float((want32.detach().double().cpu() - want64).abs().max())
    err, bar = float((got - want64).abs().max()), max(FLOOR, 4.0 * gap)
    print(f"{tag}: max |err| {err:.3e}  fp32-vs-float64 gap {gap:.3e}  bar {bar:.3e}")
    assert torch.isfinite(got).all() and err <= bar, (tag, err, gap, bar)


def torch_pair(shape, mem="gru", act="elu", seed=0, R_=R):
    from train_estimator import TerrainEstimatorTorch
    torch.manual_seed(seed)
    m32 = TerrainEstimatorTorch(shape, P, R_, memory_type=mem, activation=act)          # default widths, torch's default initialisation
    m64 = copy.deepcopy(m32).double()
    return m32, m64


# ------------------------------------------------------------------------------------------------------------ 3. the encoder alone
@pytest.mark.parametrize("shape", [(28, 56), (58, 87)], ids=["28x56", "58x87"])
@pytest.mark.parametrize("n", [1, 63, 4096])
def test_encoder_against_float64_torch(shape, n):
    from extended_legged_gym_amd.rl import NativeConvEncoder
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    m32, m64 = torch_pair(shape, seed=n)
    enc = NativeConvEncoder(parse_estimator_state(m32.state_dict(), shape, P)["encoder"], shape, device="cuda:0")
    g = torch.Generator().manual_seed(7 * n + shape[0])
    fifo = torch.rand(n, 3, *shape, generator=g)                     # the latest frame of a 3-deep FIFO: depth_stride = 3 h w
    dev = fifo.cuda()
    got = enc(dev)
    assert dev[:, -1].data_ptr() != dev.data_ptr() and not dev[:, -1].is_contiguous() or n == 1
    with torch.no_grad():
        want64, want32 = m64.encode(fifo[:, -1].double()), m32.encode(fifo[:, -1])
    check(f"encoder {shape} n={n}", got, want64, want32)
    again = enc(dev)
    assert torch.equal(got, again), "the same call twice must give the same bits"
    # the other frames of the FIFO are not what is read
    dev2 = dev.clone()
    dev2[:, :-1] += 1.0
    assert torch.equal(enc(dev2), got)
    enc.close()


# ------------------------------------------------------------------------------------------------------------ 4. the golden cases
def _golden_cases():
    from train_estimator import GOLDEN_CASES
    return GOLDEN_CASES


@pytest.mark.parametrize("index", range(5), ids=["gru_28x56", "lstm_28x56", "gru_58x87", "relu_28x56", "tanh_28x56"])
def test_estimator_step_on_the_golden_cases(index):
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    from train_estimator import TerrainEstimatorTorch, closed_form_depth, closed_form_state
    case = _golden_cases()[index]
    name, shape, mem, act = case
    m = TerrainEstimatorTorch(shape, P, R, memory_type=mem, activation=act)
    est = NativeTerrainEstimator(closed_form_state(m, salt=index), shape, P, activation=act, memory_type=mem, device="cuda:0")
    assert est.num_raycast_outputs == R and est.spec["memory_hidden_size"] == 256
    depth = closed_form_depth(T, N, *shape).cuda()
    proprio, dones = torch.from_numpy(G[name + "/proprio"]).cuda(), torch.from_numpy(G[name + "/dones"]).cuda()
    bar_p, bar_h = (max(FLOOR, 4.0 * g) for g in G[name + "/gap"])
    for t in range(T):
        pred = est.act_inference(depth[t], proprio[t])
        h = est.get_hidden_states()
        h = torch.stack(list(h) if isinstance(h, tuple) else [h])
        err_p = float((pred.cpu() - torch.from_numpy(G[name + "/predictions"][t])).abs().max())
        err_h = float((h.cpu() - torch.from_numpy(G[name + "/hidden"][t])).abs().max())
        print(f"{name} step {t}: predictions err {err_p:.3e} (gap {G[name + '/gap'][0]:.3e}, bar {bar_p:.3e}); hidden err {err_h:.3e} (gap {G[name + '/gap'][1]:.3e}, bar {bar_h:.3e})")
        assert err_p <= bar_p and err_h <= bar_h, (name, t, err_p, err_h)
        est.reset(dones[t])
    est.close()


def test_reset_rows_of_the_step_equal_a_reset_after_the_step():
    """`lg_estimator_step`'s `reset` argument (rows enter with zero state) against `reset(dones)` between two steps."""
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    from train_estimator import TerrainEstimatorTorch, closed_form_depth, closed_form_state
    m = TerrainEstimatorTorch((28, 56), P, R, memory_type="lstm")
    sd = closed_form_state(m, salt=1)
    a, b = (NativeTerrainEstimator(sd, (28, 56), P, memory_type="lstm", device="cuda:0") for _ in range(2))
    depth, proprio = closed_form_depth(2, N, 28, 56).cuda(), torch.from_numpy(G["lstm_28x56/proprio"]).cuda()
    dones = torch.tensor([1, 0, 0, 1, 0, 0, 0, 1.0]).cuda()
    a.act_inference(depth[0], proprio[0]); b.act_inference(depth[0], proprio[0])
    a.reset(dones)
    pa, pb = a.act_inference(depth[1], proprio[1]), b._step(depth[1], proprio[1], dones)
    assert torch.equal(pa, pb) and all(torch.equal(x, y) for x, y in zip(a.get_hidden_states(), b.get_hidden_states()))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ 5. full size
def test_full_size_against_float64_torch():
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    n = 4096
    m32, m64 = torch_pair((28, 56), seed=3, R_=512)
    est = NativeTerrainEstimator(m32.state_dict(), (28, 56), P, device="cuda:0")
    g = torch.Generator().manual_seed(11)
    for t in range(6):
        depth, proprio = torch.rand(n, 28, 56, generator=g), torch.randn(n, P, generator=g)
        dones = (torch.rand(n, generator=g) < 0.05).float()
        got = est.act_inference(depth.cuda(), proprio.cuda())
        with torch.no_grad():
            want64, want32 = m64.act_inference(depth.double(), proprio.double()), m32.act_inference(depth, proprio)
        check(f"full size step {t} predictions", got, want64, want32)
        check(f"full size step {t} hidden", est.get_hidden_states(), m64.get_hidden_states(), m32.get_hidden_states())
        est.reset(dones.cuda()); m32.reset(dones); m64.reset(dones)
    est.close()


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_a_status_and_a_message():
    from extended_legged_gym_amd.rl import NativeMLP, NativeTerrainEstimator
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    m32, _ = torch_pair((28, 56))
    with pytest.raises(ValueError, match="depth_image_shape"):
        NativeTerrainEstimator(m32.state_dict(), (129, 56), P, device="cuda:0")
    with pytest.raises(ValueError, match=r"combination_mlp\.0\.weight"):
        NativeTerrainEstimator(m32.state_dict(), (28, 56), P + 1, device="cuda:0")
    est = NativeTerrainEstimator(m32.state_dict(), (28, 56), P, device="cuda:0")
    lib, enc = est.encoder.lib, est.encoder
    msg = lambda: (lib.lg_mlp_last_error(None) or b"").decode()          # noqa: E731
    # the C side refuses the image size on its own, whatever Python checked
    fp = C.POINTER(C.c_float)
    spec = parse_estimator_state(m32.state_dict(), (28, 56), P)
    wp = (fp * 6)(*[w.ctypes.data_as(fp) for w, _ in spec["encoder"]])
    bp = (fp * 6)(*[b.ctypes.data_as(fp) for _, b in spec["encoder"]])
    assert not lib.lg_conv_encoder_create(28, 200, 64, 0, wp, bp, 0) and "image size" in msg()
    x, y = torch.zeros(4, 28, 56, device="cuda"), torch.full((4, 64), 7.0, device="cuda")
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.lg_conv_encoder_forward(enc.handle, px, 1568, 0, py, None) == abi.LG_ERR_INVALID and "n must be positive" in msg()
    assert lib.lg_conv_encoder_forward(enc.handle, None, 1568, 4, py, None) == abi.LG_ERR_INVALID and "null" in msg()
    assert lib.lg_conv_encoder_forward(enc.handle, px, 1567, 4, py, None) == abi.LG_ERR_INVALID and "depth_stride" in msg()
    h = torch.zeros(1, 4, 256, device="cuda")
    pr, out = torch.zeros(4, P, device="cuda"), torch.full((4, R), 7.0, device="cuda")
    args = lambda **k: [k.get("enc", enc.handle), k.get("comb", est.combine.handle), est.memory.handle, k.get("dec", est.decoder.handle), px, 1568,   # noqa: E731
                        k.get("proprio", C.c_void_p(pr.data_ptr())), k.get("n", 4), C.c_void_p(h.data_ptr()), None, None, C.c_void_p(out.data_ptr()), None]
    assert lib.lg_estimator_step(*args(n=0)) == abi.LG_ERR_INVALID and "n must be positive" in msg()
    assert lib.lg_estimator_step(*args(proprio=None)) == abi.LG_ERR_INVALID and "proprio" in msg()
    assert lib.lg_estimator_step(*args(comb=est.decoder.handle)) == abi.LG_ERR_INVALID and "widths do not chain" in msg()
    wrong = NativeMLP([(np.zeros((5, 100), np.float32), np.zeros(5, np.float32))], device="cuda:0")          # decoder of the wrong input width
    assert lib.lg_estimator_step(*args(dec=wrong.handle)) == abi.LG_ERR_INVALID and "widths do not chain" in msg()
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(out.min()) == 7.0, "a refused call must not launch"
    wrong.close(); est.close()


def test_trailing_activation_is_opt_in():
    """`lg_mlp_set_output_activation`: existing callers keep a linear last layer; the switch adds the activation and nothing else."""
    from extended_legged_gym_amd.rl import NativeMLP
    rng = np.random.default_rng(0)
    layers = [(rng.standard_normal((40, 70)).astype(np.float32) * 0.3, rng.standard_normal(40).astype(np.float32))]
    mlp = NativeMLP(layers, "elu", "cuda:0")
    x = torch.from_numpy(rng.standard_normal((50, 70)).astype(np.float32)).cuda()
    lin = mlp(x)
    assert mlp.lib.lg_mlp_set_output_activation(mlp.handle, 1) == abi.LG_OK
    act = mlp(x)
    assert mlp.lib.lg_mlp_set_output_activation(mlp.handle, 0) == abi.LG_OK
    assert torch.equal(mlp(x), lin) and float(lin.min()) < -1.0
    want = torch.nn.functional.elu(lin.double())
    assert float((act.double() - want).abs().max()) <= FLOOR and torch.equal(act[lin > 0], lin[lin > 0])
    mlp.close()


# ------------------------------------------------------------------------------------------------------------ 7. collection
def _env(n=32):
    from tests.test_env_api import make
    return make("elspider_air_rough_raycast", n, **ENV_OVER)


class _ProprioPolicy:
    """A native policy for the task: its observation row is 66 + 512 wide, more than `lg_mlp`'s 512 inputs, so the actor (a `NativeMLP`) reads the
    66 proprioceptive columns.  `collect_estimation` only asks for `act_inference(env.obs_buf)`."""

    def __init__(self, env, seed=5):
        from extended_legged_gym_amd.rl import NativeMLP
        torch.manual_seed(seed)
        dims, layers = [66, 64, 32, env.num_actions], []
        for i in range(3):
            lin = torch.nn.Linear(dims[i], dims[i + 1])
            layers.append((lin.weight.detach().numpy() * 0.3, lin.bias.detach().numpy()))
        self.actor = NativeMLP(layers, "elu", "cuda:0")

    def act_inference(self, obs):
        return self.actor(obs[:, :66])


def _policy(env, seed=5):
    return _ProprioPolicy(env, seed)


@pytest.mark.parametrize("with_policy", [True, False], ids=["policy", "random"])
def test_collect_estimation_equals_a_python_loop(with_policy):
    from extended_legged_gym_amd.rl import NativeTerrainEstimator, collect_estimation
    from train_estimator import collect_python_loop
    steps, rows = 10, []
    m32, _ = torch_pair((28, 56), seed=2, R_=512)
    for native in (True, False):
        env = _env()
        env.reset()
        policy = _policy(env) if with_policy else None
        torch.manual_seed(9)
        if native:
            est = NativeTerrainEstimator(m32.state_dict(), (28, 56), P, device="cuda:0")
            rows.append(collect_estimation(env, policy, steps, estimator=est))
            est.close()
        else:
            rows.append(collect_python_loop(env, policy, steps))
        env.core.close()
    a, b = rows
    assert tuple(a["depth_images"].shape) == (steps, 32, 28, 56) and tuple(a["raycast_targets"].shape) == (steps, 32, 512) and tuple(a["proprio_data"].shape) == (steps, 32, 6)
    for k in ("depth_images", "proprio_data", "raycast_targets", "dones"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["depth_images"].std()) > 0 and float(a["raycast_targets"].max()) > 1.0          # un-normalised distances, in metres
    assert not torch.equal(a["depth_images"][0], a["depth_images"][-1])
    # the predictions equal stepping act_inference by hand over the returned rows, reset on dones after each step
    est = NativeTerrainEstimator(m32.state_dict(), (28, 56), P, device="cuda:0")
    for t in range(steps):
        pred = est.act_inference(a["depth_images"][t], a["proprio_data"][t])
        assert torch.equal(pred, a["predictions"][t]), t
        assert float(a["mse"][t]) == float(torch.mean((pred - a["raycast_targets"][t]) ** 2))
        est.reset(a["dones"][t])
    est.close()


# ------------------------------------------------------------------------------------------------------------ 8. the training tool
def test_train_tool_native_collection_equals_the_python_loop():
    """Same rows, so equal losses -- given an update that is itself reproducible: torch's convolution backward on the GPU is not (a first version of
    this test ran the update there and saw 54.2713885 against 54.2713890 at the second iteration, after one gradient step, in one of two runs), so
    the update of both runs is placed on the CPU.  Collection, the estimator built from the result and its evaluation run on the GPU."""
    from train_estimator import train
    curves = [train(3, 32, steps=8, seed=4, python_loop=loop, gradient_length=4, log=lambda s: None, small_terrain=True, update_device="cpu")
              for loop in (False, True)]
    print("estimation loss, native collection:", curves[0], " python loop:", curves[1])
    assert len(curves[0]) == 3 and all(np.isfinite(curves[0])) and curves[0] == curves[1]

"""GPU: the depth encoder in precision "bf16" (include/lgpolicy.h `lg_conv_encoder_create_precision`, LG_PREC_BF16; `NativeConvEncoder(...,
precision="bf16")`, `NativeTerrainEstimator(..., encoder_precision="bf16")`): every stage against the bf16-operand float64 reference by the
interval rule of tests/bf16_encoder_rule.py, over the shapes, inputs and weights of tests/test_encoder_reference_power.py; output widths and
activations; a workspace grown and used again; a strided FIFO; the fp32 path through the new constructor; `lg_estimator_step` on the golden
cases; `collect_estimation`.

Every `out` is one row longer than asked for and pre-filled: the row behind the last must come back untouched (stage 7 is written by the
kernel itself, stages 1-6 by the expanding copy)."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from extended_legged_gym_amd import abi
from tests.bf16_encoder_rule import R, bf16_operand_pair, check_interval, stage_reference
from tests.test_encoder_reference_power import FLOOR, SHAPES, camera_input, model_pair, run_stage, wide_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu
SENTINEL = -777.0
P, RAYS = 6, 81


def capped(shape, n):
    from tests.test_hip_encoder_stages import capped as cap
    return cap(shape, n)


def native_encoder(m32, shape, act="elu", precision="bf16"):
    from extended_legged_gym_amd.rl import NativeConvEncoder
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    return NativeConvEncoder(parse_estimator_state(m32.state_dict(), shape, m32.proprio_dim)["encoder"], shape, act, device="cuda:0", precision=precision)


def sweep_bf16(tag, enc, m32, x, dev=None):
    """All seven stages of the bf16 encoder `enc` on the images x (n, h, w; CPU) by the interval rule; the guard row; stage 7 against the full
    forward in bits; a second identical call in bits.  `dev`: the device tensor handed to the encoder (default x itself on the GPU)."""
    n = x.shape[0]
    dev = x.cuda() if dev is None else dev
    r32, r64 = bf16_operand_pair(m32)
    prev, worst = R(x).unsqueeze(1), 0.0
    for k in range(1, 8):
        count, _ = enc.stage_shape(k)
        buf = torch.full(((n + 1) * count,), SENTINEL, device="cuda")
        got = enc.stage(dev, k, out=buf)
        torch.cuda.synchronize()
        assert bool((buf[n * count:] == SENTINEL).all()), f"{tag} stage {k}: the row behind the last was written"
        got = got.cpu().contiguous()
        if k < 7:
            assert torch.equal(R(got), got), f"{tag} stage {k}: a stored value is not a bf16 value"
        u, gap, bar = stage_reference(r32, r64, k, prev)
        worst = max(worst, check_interval(tag, got, u, bar, gap, k))
        prev = got
    full = enc(dev)
    assert torch.equal(got, full.cpu()), f"{tag}: stage(x, 7) and the full forward differ in bits"
    assert torch.equal(enc(dev), full), f"{tag}: the same call twice must give the same bits"
    return full, worst


# ------------------------------------------------------------------------------------------------------------ 5. shapes x batch sizes
SWEEP = [(s, n) for s in SHAPES for n in (1, 3, 70)]


@pytest.mark.parametrize("shape,n", SWEEP, ids=[f"{s[0]}x{s[1]}-n{n}" for s, n in SWEEP])
def test_bf16_stages_over_shapes_and_batches(shape, n):
    n = capped(shape, n)
    m32, _ = model_pair(shape, salt=SHAPES.index(shape))
    enc = native_encoder(m32, shape)
    assert enc.precision == "bf16" and enc.lib.lg_conv_encoder_precision(enc.handle) == abi.LG_PREC_BF16
    full, _ = sweep_bf16(f"{shape} n={n} camera", enc, m32, camera_input(n, shape))
    assert tuple(full.shape) == (n, 64)
    if n == 3:
        sweep_bf16(f"{shape} n={n} wide", enc, m32, wide_input(n, shape))
    enc.close()


# ------------------------------------------------------------------------------------------------------------ 6. widths, activations, reuse, FIFO
@pytest.mark.parametrize("out_dim", [1, 65, 512])
@pytest.mark.parametrize("act", ["elu", "relu", "tanh"])
def test_bf16_stages_over_widths_and_activations(out_dim, act):
    shape, n = (29, 57), 3
    m32, _ = model_pair(shape, salt=out_dim, out_dim=out_dim, act=act, proprio_dim=0)
    enc = native_encoder(m32, shape, act)
    for name, x in (("camera", camera_input(n, shape)), ("wide", wide_input(n, shape))):
        full, _ = sweep_bf16(f"{shape} n={n} out_dim={out_dim} {act} {name}", enc, m32, x)
        assert tuple(full.shape) == (n, out_dim)
    enc.close()


def test_bf16_workspace_grown_then_used_at_a_smaller_n():
    shape = (29, 57)
    m32, _ = model_pair(shape, salt=2)
    used, images = native_encoder(m32, shape), {n: camera_input(n, shape) for n in (3, 70)}
    for n in (70, 3):
        fresh = native_encoder(m32, shape)
        full, _ = sweep_bf16(f"{shape} reused n={n}", used, m32, images[n])
        assert torch.equal(full, fresh(images[n].cuda())), n
        for k in (2, 5, 6):
            assert torch.equal(used.stage(images[n].cuda(), k), fresh.stage(images[n].cuda(), k)), (n, k)
        fresh.close()
    used.close()


def test_bf16_reads_the_latest_frame_of_a_strided_fifo():
    shape, n = (29, 57), 3
    m32, _ = model_pair(shape, salt=4)
    enc = native_encoder(m32, shape)
    x = camera_input(n, shape)
    fifo = torch.stack([x + 1.0, x], dim=1).cuda()          # (n, 2, h, w): depth_stride = 2 h w, the latest frame is x
    view = enc.latest_frame(fifo)
    assert view.stride(0) == 2 * shape[0] * shape[1] and view.data_ptr() != fifo.data_ptr()
    full, _ = sweep_bf16(f"{shape} n={n} FIFO", enc, m32, x, dev=fifo)
    assert torch.equal(full, enc(x.cuda()))
    enc.close()


# ------------------------------------------------------------------------------------------------------------ 7. the fp32 path
@pytest.mark.parametrize("shape", [(29, 57), (28, 56)], ids=["29x57", "28x56"])
def test_fp32_through_the_new_constructor_equals_the_old_one(shape):
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    n = 70
    m32, _ = model_pair(shape, salt=1)
    old = native_encoder(m32, shape, precision="fp32")          # lg_conv_encoder_create
    layers = parse_estimator_state(m32.state_dict(), shape, m32.proprio_dim)["encoder"]
    fp = C.POINTER(C.c_float)
    wp = (fp * 6)(*[w.ctypes.data_as(fp) for w, _ in layers])
    bp = (fp * 6)(*[b.ctypes.data_as(fp) for _, b in layers])
    lib = old.lib
    handle = lib.lg_conv_encoder_create_precision(shape[0], shape[1], 64, abi.ACTIVATIONS["elu"], wp, bp, 0, abi.LG_PREC_F32)
    assert handle and lib.lg_conv_encoder_precision(handle) == abi.LG_PREC_F32 and lib.lg_conv_encoder_precision(old.handle) == abi.LG_PREC_F32
    new = copy.copy(old)
    new.handle = handle
    x = camera_input(n, shape).cuda()
    for k in range(1, 8):
        assert torch.equal(old.stage(x, k), new.stage(x, k)), k
    assert torch.equal(old(x), new(x))
    assert not lib.lg_conv_encoder_create_precision(shape[0], shape[1], 64, 0, wp, bp, 0, 2)
    assert "precision" in (lib.lg_mlp_last_error(None) or b"").decode()
    new.close(); old.close()


# ------------------------------------------------------------------------------------------------------------ 8. the estimator, end to end
G = np.load(os.path.join(ROOT, "tests", "golden", "terrain_estimator.npz"))
T, N = 6, 8


def emulate_bf16(index):
    """CPU float64 emulation of the estimator with a bf16 encoder on golden case `index`: encoder weights and image through R, the output of
    stages 1-6 through R, everything else float64.  Returns predictions (T, N, RAYS) and hidden (T, layers-or-2, N, H) as the golden file has them."""
    from train_estimator import GOLDEN_CASES, TerrainEstimatorTorch, closed_form_depth, closed_form_state
    name, shape, mem, act = GOLDEN_CASES[index]
    m = TerrainEstimatorTorch(shape, P, RAYS, memory_type=mem, activation=act)
    m.load_state_dict(closed_form_state(m, salt=index))
    _, r64 = bf16_operand_pair(m)
    depth = closed_form_depth(T, N, *shape)
    proprio, dones = torch.from_numpy(G[name + "/proprio"]).double(), torch.from_numpy(G[name + "/dones"])
    preds, hidden = [], []
    with torch.no_grad():
        for t in range(T):
            x = R(depth[t]).double().unsqueeze(1)
            for k in range(1, 8):
                x = run_stage(r64, k, x)
                if k < 7:
                    x = R(x)
            preds.append(r64.decoder(r64.memory(r64.combination_mlp(torch.cat([x, proprio[t]], dim=-1)))))
            h = r64.get_hidden_states()
            hidden.append(torch.stack(list(h) if isinstance(h, tuple) else [h]))
            r64.reset(dones[t])
    return torch.stack(preds), torch.stack(hidden)


@pytest.mark.parametrize("index", range(5), ids=["gru_28x56", "lstm_28x56", "gru_58x87", "relu_28x56", "tanh_28x56"])
def test_bf16_estimator_step_on_the_golden_cases(index):
    """Bar per case and quantity = max(the fp32 bar of tests/test_hip_estimator.py, 3 x the deviation of the float64 bf16-operand emulation
    from the golden arrays, the worst over the case's steps)."""
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    from train_estimator import GOLDEN_CASES, TerrainEstimatorTorch, closed_form_depth, closed_form_state
    name, shape, mem, act = GOLDEN_CASES[index]
    emu_p, emu_h = emulate_bf16(index)
    gold_p, gold_h = torch.from_numpy(G[name + "/predictions"]).double(), torch.from_numpy(G[name + "/hidden"]).double()
    assert emu_p.shape == gold_p.shape and emu_h.shape == gold_h.shape, (emu_p.shape, gold_p.shape, emu_h.shape, gold_h.shape)
    dev_p, dev_h = (emu_p - gold_p).abs().flatten(1).max(1).values, (emu_h - gold_h).abs().flatten(1).max(1).values
    fp32_p, fp32_h = (max(FLOOR, 4.0 * g) for g in G[name + "/gap"])
    bar_p, bar_h = max(fp32_p, 3.0 * float(dev_p.max())), max(fp32_h, 3.0 * float(dev_h.max()))
    m = TerrainEstimatorTorch(shape, P, RAYS, memory_type=mem, activation=act)
    est = NativeTerrainEstimator(closed_form_state(m, salt=index), shape, P, activation=act, memory_type=mem, device="cuda:0", encoder_precision="bf16")
    assert est.precision == "bf16" and est.encoder.precision == "bf16"
    depth = closed_form_depth(T, N, *shape).cuda()
    proprio, dones = torch.from_numpy(G[name + "/proprio"]).cuda(), torch.from_numpy(G[name + "/dones"]).cuda()
    worst = 0.0
    for t in range(T):
        pred = est.act_inference(depth[t], proprio[t])
        h = est.get_hidden_states()
        h = torch.stack(list(h) if isinstance(h, tuple) else [h])
        err_p, err_h = float((pred.cpu().double() - gold_p[t]).abs().max()), float((h.cpu().double() - gold_h[t]).abs().max())
        worst = max(worst, err_p / bar_p, err_h / bar_h)
        print(f"{name} step {t}: predictions err {err_p:.3e} (emulation {float(dev_p[t]):.3e}, bar {bar_p:.3e}); "
              f"hidden err {err_h:.3e} (emulation {float(dev_h[t]):.3e}, bar {bar_h:.3e})")
        assert torch.isfinite(pred).all() and err_p <= bar_p and err_h <= bar_h, (name, t, err_p, bar_p, err_h, bar_h)
        est.reset(dones[t])
    print(f"{name}: worst err / bar {worst:.3f}")
    est.close()


def test_bf16_refusals_leave_a_status_and_launch_nothing():
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    shape = (28, 56)
    m32, _ = model_pair(shape)
    est = NativeTerrainEstimator(m32.state_dict(), shape, P, device="cuda:0", encoder_precision="bf16")
    lib, enc = est.encoder.lib, est.encoder
    msg = lambda: (lib.lg_mlp_last_error(None) or b"").decode()          # noqa: E731
    x, y = torch.zeros(4, 28, 56, device="cuda"), torch.full((4 * 14 * 28 * 32,), 7.0, device="cuda")
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.lg_conv_encoder_forward(enc.handle, px, 1568, 0, py, None) == abi.LG_ERR_INVALID and "n must be positive" in msg()
    assert lib.lg_conv_encoder_forward(enc.handle, None, 1568, 4, py, None) == abi.LG_ERR_INVALID and "null" in msg()
    assert lib.lg_conv_encoder_forward(enc.handle, px, 1567, 4, py, None) == abi.LG_ERR_INVALID and "depth_stride" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1567, 4, 1, py, None) == abi.LG_ERR_INVALID and "depth_stride" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1568, 4, 8, py, None) == abi.LG_ERR_INVALID and "stages must be 1..7" in msg()
    h = torch.full((1, 4, 256), 7.0, device="cuda")
    pr, out = torch.zeros(4, P, device="cuda"), torch.full((4, RAYS), 7.0, device="cuda")
    args = lambda **k: [enc.handle, est.combine.handle, est.memory.handle, est.decoder.handle, k.get("depth", px), k.get("stride", 1568),   # noqa: E731
                        k.get("proprio", C.c_void_p(pr.data_ptr())), k.get("n", 4), k.get("h", C.c_void_p(h.data_ptr())), None, None,
                        k.get("out", C.c_void_p(out.data_ptr())), None]
    for kw, word in ((dict(n=0), "n must be positive"), (dict(n=-3), "n must be positive"), (dict(depth=None), "null"), (dict(h=None), "null"),
                     (dict(out=None), "null"), (dict(proprio=None), "proprio"), (dict(stride=1567), "depth_stride")):
        assert lib.lg_estimator_step(*args(**kw)) == abi.LG_ERR_INVALID and word in msg(), (kw, msg())
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(out.min()) == 7.0 and float(h.min()) == 7.0, "a refused call must not launch"
    est.close()


# ------------------------------------------------------------------------------------------------------------ 9. collection
def test_bf16_collect_estimation_equals_a_python_loop():
    from extended_legged_gym_amd.rl import NativeTerrainEstimator, collect_estimation
    from tests.test_hip_estimator import _env, torch_pair
    from train_estimator import collect_python_loop
    steps, rows = 6, []
    m32, _ = torch_pair((28, 56), seed=2, R_=512)
    for native in (True, False):
        env = _env()
        env.reset()
        torch.manual_seed(9)
        if native:
            est = NativeTerrainEstimator(m32.state_dict(), (28, 56), 6, device="cuda:0", encoder_precision="bf16")
            rows.append(collect_estimation(env, None, steps, estimator=est))
            est.close()
        else:
            rows.append(collect_python_loop(env, None, steps))
        env.core.close()
    a, b = rows
    for k in ("depth_images", "proprio_data", "raycast_targets", "dones"):
        assert torch.equal(a[k], b[k]), k
    est = NativeTerrainEstimator(m32.state_dict(), (28, 56), 6, device="cuda:0", encoder_precision="bf16")
    fp32 = NativeTerrainEstimator(m32.state_dict(), (28, 56), 6, device="cuda:0")
    for t in range(steps):
        pred = est.act_inference(a["depth_images"][t], a["proprio_data"][t])
        assert torch.equal(pred, a["predictions"][t]), t
        assert float(a["mse"][t]) == float(torch.mean((pred - a["raycast_targets"][t]) ** 2))
        assert not torch.equal(pred, fp32.act_inference(a["depth_images"][t], a["proprio_data"][t])), "the bf16 encoder did not run"
        est.reset(a["dones"][t]); fp32.reset(a["dones"][t])
    est.close(); fp32.close()

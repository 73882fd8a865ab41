"""GPU: the depth encoder of the terrain estimator stage by stage (include/lgpolicy.h `lg_conv_encoder_forward_stages`; `NativeConvEncoder.stage`)
against `tools/train_estimator.TerrainEstimatorTorch` in float64 cut after the matching module of `depth_encoder`, over image sizes, batch
sizes, output widths and activations; workspaces that grow and are used again at a smaller n; `lg_estimator_step` away from the default widths.

Why per stage: tests/test_encoder_reference_power.py (no GPU) shows on these same inputs and weights that a wrong tap, border, bias column or env
moves the map of its own stage by at least ten bars -- by thousands for most -- while AdaptiveAvgPool2d and two linear layers can shrink it
under the end-to-end bar of tests/test_hip_estimator.py.  Shapes, inputs, weights and the bar come from that file.

Tolerance: the rule of tests/test_hip_estimator.py at every stage k, not a new number: max(2e-5, 4 x gap_k), gap_k = torch fp32 against torch
float64 at that stage.  Each case prints stage, error, gap and bar; a failure names the env, (y, x, channel) and whether the pixel is on the border.

Every `out` is one row longer than asked for and pre-filled: the row behind the last must come back untouched.  What that can catch: at stage 7
the kernel writes `out` itself, so a column >= out_dim of the LAST row, or a row >= n of the last 64-row tile, lands there (an overrun of an
earlier row lands in the next row and shows as an error of that row instead); at stages 1-6 the kernels write the encoder's workspaces and `out`
is filled by a copy, so there the guard checks the copy's length only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from extended_legged_gym_amd import abi
from tests.test_encoder_reference_power import (FLOOR, P, R, SHAPES, STAGE_NAMES, camera_input, conv4_side, model_pair, stage_bars, wide_input)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu
SENTINEL = -777.0
MAP_BYTES = 64 << 20          # at the two largest shapes the conv 1 map of one call stays under this
LARGEST = SHAPES[-2:]


def check_close(tag, got, want64, gap, stage=None):
    """The one failure report: worst entry's env and position.  `got` / `want64`: (n, C, H, W) maps or (rows, width) rows -- for a hidden state
    (layers, n, H) flattened to (layers n, H), row = layer n + env.  Returns err / bar."""
    got, want64 = got.detach().double().cpu(), want64.detach().double().cpu()
    assert got.shape == want64.shape, (tag, tuple(got.shape), tuple(want64.shape))
    diff = (got - want64).abs()
    diff[~torch.isfinite(got)] = float("inf")
    err, bar = float(diff.max()), max(FLOOR, 4.0 * gap)
    idx = np.unravel_index(int(diff.argmax()), tuple(diff.shape))
    if got.dim() == 4:
        e, c, y, x = (int(v) for v in idx)
        where = f"env {e} (y, x, channel) = ({y}, {x}, {c}) of a {got.shape[2]} x {got.shape[3]} map, " + \
                ("on its border" if y in (0, got.shape[2] - 1) or x in (0, got.shape[3] - 1) else "interior")
    else:
        assert got.dim() == 2, (tag, tuple(got.shape))
        where = f"row {int(idx[0])} of {got.shape[0]}, column {int(idx[1])} of {got.shape[1]}"
    name = f" stage {stage} ({STAGE_NAMES[stage - 1]})" if stage else ""
    print(f"{tag}{name}: max |err| {err:.3e}  fp32-vs-float64 gap {gap:.3e}  bar {bar:.3e}  ratio {err / bar:.4f}")
    assert err <= bar, f"{tag}{name}: |err| {err:.3e} > bar {bar:.3e} (gap {gap:.3e}) at {where}: got {float(got[idx])!r}, float64 torch {float(want64[idx])!r}"
    return err / bar


def capped(shape, n):
    """n, cut at the two largest shapes only so that their conv 1 map stays under MAP_BYTES; every other shape runs the n it is given."""
    if shape not in LARGEST:
        return n
    h, w = ((v + 4 - 5) // 2 + 1 for v in shape)
    return max(1, min(n, MAP_BYTES // (h * w * 32 * 4)))


def native_encoder(m32, shape, act="elu"):
    from extended_legged_gym_amd.rl import NativeConvEncoder
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    return NativeConvEncoder(parse_estimator_state(m32.state_dict(), shape, m32.proprio_dim)["encoder"], shape, act, device="cuda:0")


def sweep_stages(tag, enc, m32, m64, x):
    """All seven stages of `enc` on the images x (n, h, w; CPU) against float64 torch; the guard row; stage 7 against the full forward."""
    n, dev = x.shape[0], x.cuda()
    s64, gaps, _ = stage_bars(m32, m64, x)
    for k in range(1, 8):
        count, (h, w, c) = enc.stage_shape(k)
        assert count == s64[k - 1][0].numel() and (k > 4 or (c, h, w) == tuple(s64[k - 1].shape[1:])), (k, count, (h, w, c), tuple(s64[k - 1].shape))
        buf = torch.full(((n + 1) * count,), SENTINEL, device="cuda")
        got = enc.stage(dev, k, out=buf)
        torch.cuda.synchronize()
        assert bool((buf[n * count:] == SENTINEL).all()), f"{tag} stage {k}: the row behind the last was written"
        check_close(tag, got, s64[k - 1], gaps[k - 1], stage=k)
    full = enc(dev)
    assert torch.equal(got, full), f"{tag}: stage(x, 7) and the full forward differ in bits"
    return full


# ------------------------------------------------------------------------------------------------------------ shapes x batch sizes
SWEEP = [(s, n) for s in SHAPES for n in (1, 3, 70)] + [((28, 56), 4096)]


def test_the_shape_list_reaches_every_pooling_regime():
    sides = {conv4_side(v) for s in SHAPES for v in s}
    assert {1, 2, 3} <= sides and any(v >= 4 and v % 4 for v in sides), sides
    assert LARGEST == [(127, 128), (128, 128)] and all(capped(s, 10 ** 6) * 64 * 64 * 128 <= MAP_BYTES for s in LARGEST)
    assert all(capped(s, n) == n for s, n in SWEEP), "no case of the sweep is cut: 70 envs of the largest map are 37 MB, and 28 x 56 runs its 4096"
    assert ((28, 56), 4096) in SWEEP


@pytest.mark.parametrize("shape,n", SWEEP, ids=[f"{s[0]}x{s[1]}-n{n}" for s, n in SWEEP])
def test_stages_over_shapes_and_batches(shape, n):
    asked, n = n, capped(shape, n)
    assert n == asked or shape in LARGEST
    m32, m64 = model_pair(shape, salt=SHAPES.index(shape))
    enc = native_encoder(m32, shape)
    full = sweep_stages(f"{shape} n={n} camera", enc, m32, m64, camera_input(n, shape))
    assert full.shape[0] == n
    if n == 3:
        sweep_stages(f"{shape} n={n} wide", enc, m32, m64, wide_input(n, shape))
    enc.close()


def test_stages_with_torchs_default_initialisation():
    shape, n = (29, 57), 70
    m32, m64 = model_pair(shape, salt=5, default_init=True)
    enc = native_encoder(m32, shape)
    sweep_stages(f"{shape} n={n} default init", enc, m32, m64, camera_input(n, shape))
    enc.close()


# ------------------------------------------------------------------------------------------------------------ output widths, activations
@pytest.mark.parametrize("shape", [(28, 56), (29, 57)], ids=["28x56", "29x57"])
@pytest.mark.parametrize("out_dim", [1, 63, 64, 65, 512])
def test_stages_over_output_widths(shape, out_dim):
    n = 70
    m32, m64 = model_pair(shape, salt=out_dim, out_dim=out_dim, proprio_dim=0)
    enc = native_encoder(m32, shape)
    assert enc.out_dim == out_dim and enc.stage_shape(7) == (out_dim, (1, 1, out_dim))
    full = sweep_stages(f"{shape} n={n} out_dim={out_dim}", enc, m32, m64, camera_input(n, shape))
    assert tuple(full.shape) == (n, out_dim)
    enc.close()


@pytest.mark.parametrize("shape", [(28, 56), (29, 57)], ids=["28x56", "29x57"])
@pytest.mark.parametrize("act", ["elu", "relu", "tanh"])
def test_stages_over_activations(shape, act):
    n = 70
    m32, m64 = model_pair(shape, salt=11, act=act)
    enc = native_encoder(m32, shape, act)
    for name, x in (("camera", camera_input(n, shape)), ("wide", wide_input(n, shape))):
        sweep_stages(f"{shape} n={n} {act} {name}", enc, m32, m64, x)
    enc.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_stage_refusals_leave_a_status_and_launch_nothing():
    shape = (28, 56)
    m32, _ = model_pair(shape)
    enc = native_encoder(m32, shape)
    lib = enc.lib
    msg = lambda: (lib.lg_mlp_last_error(None) or b"").decode()          # noqa: E731
    x, y = torch.zeros(4, 28, 56, device="cuda"), torch.full((4 * 28 * 14 * 32,), SENTINEL, device="cuda")
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    for stages in (0, 8, -1):
        assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1568, 4, stages, py, None) == abi.LG_ERR_INVALID and "stages must be 1..7" in msg()
        assert lib.lg_conv_encoder_stage_shape(enc.handle, stages, None, None, None) == abi.LG_ERR_INVALID and "stage" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1568, 0, 1, py, None) == abi.LG_ERR_INVALID and "n must be positive" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, None, 1568, 4, 1, py, None) == abi.LG_ERR_INVALID and "null" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1568, 4, 1, None, None) == abi.LG_ERR_INVALID and "null" in msg()
    assert lib.lg_conv_encoder_forward_stages(enc.handle, px, 1567, 4, 1, py, None) == abi.LG_ERR_INVALID and "depth_stride" in msg()
    torch.cuda.synchronize()
    assert float(y.max()) == SENTINEL, "a refused call must not launch"
    assert [enc.stage_shape(k)[0] for k in range(1, 8)] == [14 * 28 * 32, 7 * 14 * 64, 4 * 7 * 128, 4 * 7 * 64, 1024, 128, 64]
    with pytest.raises(ValueError, match="stage"):
        enc.stage_shape(8)
    enc.close()


# ------------------------------------------------------------------------------------------------------------ workspaces that grow and are reused
def test_an_encoder_reused_at_a_smaller_n_equals_a_fresh_one():
    shape = (29, 57)
    m32, m64 = model_pair(shape, salt=2)
    used, images = native_encoder(m32, shape), {n: camera_input(n, shape) for n in (3, 70)}
    for n in (3, 70, 3):
        fresh = native_encoder(m32, shape)
        for k in (2, 4, 5, 7):
            assert torch.equal(used.stage(images[n].cuda(), k), fresh.stage(images[n].cuda(), k)), (n, k)
        assert torch.equal(used(images[n].cuda()), fresh(images[n].cuda())), n
        fresh.close()
        sweep_stages(f"{shape} reused n={n}", used, m32, m64, images[n])
    used.close()


def test_two_encoders_of_different_sizes_interleaved():
    a_shape, b_shape = (20, 24), (58, 87)
    (a32, a64), (b32, b64) = model_pair(a_shape, salt=3), model_pair(b_shape, salt=4)
    a, b = native_encoder(a32, a_shape), native_encoder(b32, b_shape)
    first = {}
    for turn, n in enumerate((70, 3, 70)):
        for tag, enc, m32, m64, shape in (("a", a, a32, a64, a_shape), ("b", b, b32, b64, b_shape)):
            full = sweep_stages(f"interleaved {tag} {shape} n={n} turn {turn}", enc, m32, m64, camera_input(n, shape))
            assert torch.equal(first.setdefault((tag, n), full), full), (tag, n, turn)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ the estimator step
def _hidden(h):
    return torch.stack(list(h)) if isinstance(h, tuple) else h


def _step_inputs(t, n, shape, proprio_dim):
    from train_estimator import closed_form_depth
    g = torch.Generator().manual_seed(100 * t + n)
    return closed_form_depth(t + 1, n, *shape)[t] - 0.5, torch.randn(n, proprio_dim, generator=g), (torch.rand(n, generator=g) < 0.3).float()


def test_estimator_reused_at_a_smaller_n_after_reset():
    """`act_inference` at n = 8, 200, 8 on one estimator, `reset()` between the changes: predictions and hidden state against float64 torch."""
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    shape = (28, 56)
    m32, m64 = model_pair(shape, salt=6)
    est = NativeTerrainEstimator(m32.state_dict(), shape, P, device="cuda:0")
    for n in (8, 200, 8):
        est.reset(); m32.reset(); m64.reset()
        for t in range(2):
            depth, proprio, dones = _step_inputs(t, n, shape, P)
            got = est.act_inference(depth.cuda(), proprio.cuda())
            with torch.no_grad():
                want64, want32 = m64.act_inference(depth.double(), proprio.double()), m32.act_inference(depth, proprio)
            check_close(f"estimator n={n} step {t} predictions", got, want64, float((want32.double() - want64).abs().max()))
            h64, h32 = _hidden(m64.get_hidden_states()), _hidden(m32.get_hidden_states())
            check_close(f"estimator n={n} step {t} hidden", _hidden(est.get_hidden_states()).flatten(0, 1), h64.flatten(0, 1), float((h32.double() - h64).abs().max()))
            est.reset(dones.cuda()); m32.reset(dones); m64.reset(dones)
    est.close()


STEP_SETTINGS = {"out65_proprio6": dict(out_dim=65), "out64_proprio0": dict(proprio_dim=0), "two_memory_layers": dict(memory_num_layers=2),
                 "hidden96": dict(memory_hidden_size=96), "decoder_one_layer": dict(decoder_hidden_dims=()), "decoder_130": dict(decoder_hidden_dims=(130,))}


@pytest.mark.parametrize("name", list(STEP_SETTINGS))
def test_estimator_step_away_from_the_default_widths(name):
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    shape, n, kw = (29, 57), 70, dict(STEP_SETTINGS[name])
    pd = kw.get("proprio_dim", P)
    m32, m64 = model_pair(shape, salt=7, **kw)
    est = NativeTerrainEstimator(m32.state_dict(), shape, pd, device="cuda:0")
    assert est.spec["encoder_output_dim"] == kw.get("out_dim", 64) and est.spec["memory_hidden_size"] == kw.get("memory_hidden_size", 256)
    assert est.spec["memory_num_layers"] == kw.get("memory_num_layers", 1) and tuple(est.spec["decoder_hidden_dims"]) == tuple(kw.get("decoder_hidden_dims", (128, 64)))
    for t in range(3):
        depth, proprio, dones = _step_inputs(t, n, shape, pd)
        got = est.act_inference(depth.cuda(), proprio.cuda())
        with torch.no_grad():
            want64, want32 = m64.act_inference(depth.double(), proprio.double()), m32.act_inference(depth, proprio)
        check_close(f"{name} step {t} predictions", got, want64, float((want32.double() - want64).abs().max()))
        h64, h32 = _hidden(m64.get_hidden_states()), _hidden(m32.get_hidden_states())
        check_close(f"{name} step {t} hidden", _hidden(est.get_hidden_states()).flatten(0, 1), h64.flatten(0, 1), float((h32.double() - h64).abs().max()))
        est.reset(dones.cuda()); m32.reset(dones); m64.reset(dones)
    est.close()


def test_a_combination_layer_wider_than_lg_mlp_is_refused_by_name():
    """encoder_output_dim 512 + proprio_dim 6 = 518 inputs, more than an lg_mlp layer takes: a Python exception that names the width, before any
    native object exists -- not a launch, not a truncation.  (Before this check the same state failed in `lg_mlp_create` with "layer width out of
    range (1..512)": an exception too, but one that did not say which layer or how wide.)"""
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    from extended_legged_gym_amd.rl.estimator import parse_estimator_state
    m32, _ = model_pair((28, 56), out_dim=512)
    with pytest.raises(ValueError, match=r"512 \+ proprio_dim 6 = 518 inputs"):
        parse_estimator_state(m32.state_dict(), (28, 56), P)
    with pytest.raises(ValueError, match="518"):
        NativeTerrainEstimator(m32.state_dict(), (28, 56), P, device="cuda:0")
    m0, m0_64 = model_pair((28, 56), out_dim=512, proprio_dim=0)          # 512 + 0 is the widest that runs
    est = NativeTerrainEstimator(m0.state_dict(), (28, 56), 0, device="cuda:0")
    depth, proprio, _ = _step_inputs(0, 5, (28, 56), 0)
    got = est.act_inference(depth.cuda(), proprio.cuda())
    with torch.no_grad():
        want64, want32 = m0_64.act_inference(depth.double(), proprio.double()), m0.act_inference(depth, proprio)
    check_close("out_dim 512, proprio 0 predictions", got, want64, float((want32.double() - want64).abs().max()))
    est.close()

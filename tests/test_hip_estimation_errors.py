"""GPU: `lg_estimation_errors` alone (include/lgrunner_estimator.h; `estimation_error_kernel` and its finish in csrc/lg_runner_estimator.hip) -- the
per-step MSE / MAE of the estimator's predictions and the four per-ray rows accumulated over the steps of a call.

Shapes: 3 x 25 (the scalar path, a tail of lanes past the last ray), 33 x 512 over three steps (the 16-byte path, two tiles of column units, nine
row slabs, the rows accumulated across steps), 5 x 28 with every pointer shifted by one float (a width that would take 16-byte loads on pointers that
do not), 4096 x 512 (1024 blocks of four rows on the capped grid of 128 slabs: the grid-stride loop turns eight times).

Against float64 on the CPU of the same rows every figure is held to max(2e-5, 4 x yardstick) relative, the yardstick being torch's own fp32
(`torch.mean`, `sum(dim=0)`) against that float64, measured here: the rule of tests/test_hip_policy_sweep.py.  The running maximum is exact.
Guard floats around every output stay untouched, and two runs give equal bits.  Each comparison prints its figure before it asserts."""
import ctypes as C

import pytest
import torch

from extended_legged_gym_amd import abi

pytestmark = pytest.mark.gpu
FLOOR = 2e-5
GUARD = 8
CASES = [(3, 25, 1, 0), (33, 512, 3, 0), (5, 28, 2, 1), (4096, 512, 2, 0)]
IDS = ["scalar_with_tail", "vector_accumulating", "vector_width_unaligned_pointers", "grid_stride_turns"]


def _guarded(count, shift, fill=-7.0):
    buf = torch.full((count + 2 * GUARD + shift,), fill, device="cuda")
    return buf, buf[GUARD + shift: GUARD + shift + count]


def _run(lib, pred, tgt, steps, n, R, shift):
    floats = int(lib.lg_estimation_errors_workspace(n, R))
    bufs = {k: _guarded(c, shift) for k, c in (("mse", steps), ("mae", steps), ("ray_sq_error", R), ("ray_abs_error", R), ("ray_bias", R), ("ray_max_error", R),
                                                 ("workspace", floats))}
    stats = abi.lg_estimation_stats(workspace_floats=floats, **{k: v[1].data_ptr() for k, v in bufs.items()})
    rc = lib.lg_estimation_errors(C.c_void_p(pred.data_ptr()), C.c_void_p(tgt.data_ptr()), steps, n, R, C.byref(stats), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (lib.lg_mlp_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("n,R,steps,shift", CASES, ids=IDS)
def test_error_figures_against_float64(n, R, steps, shift):
    from extended_legged_gym_amd.rl.estimator_runner import _estimator_lib
    lib = _estimator_lib()
    g = torch.Generator(device="cuda").manual_seed(1000 * n + R)
    pb, pred = _guarded(steps * n * R, shift, 0.0)
    tb, tgt = _guarded(steps * n * R, shift, 0.0)
    pred.copy_(torch.randn(steps * n * R, device="cuda", generator=g) * 5)
    tgt.copy_(torch.randn(steps * n * R, device="cuda", generator=g).abs() * 5)
    assert (pred.data_ptr() % 16 != 0) == bool(shift)
    first, second = _run(lib, pred, tgt, steps, n, R, shift), _run(lib, pred, tgt, steps, n, R, shift)
    for key, (buf, view) in first.items():
        if key == "workspace":
            continue
        count = view.numel()
        assert bool((buf[:GUARD + shift] == -7.0).all()) and bool((buf[GUARD + shift + count:] == -7.0).all()), f"{key}: a guard float moved"
        assert torch.equal(view, second[key][1]), f"{key}: two runs differ"
    p32, t32 = pred.view(steps, n, R).cpu(), tgt.view(steps, n, R).cpu()
    d32, d64 = p32 - t32, p32.double() - t32.double()
    want = dict(mse=(d64 ** 2).mean(dim=(1, 2)), mae=d64.abs().mean(dim=(1, 2)), ray_sq_error=(d64 ** 2).sum(dim=(0, 1)), ray_abs_error=d64.abs().sum(dim=(0, 1)),
                ray_bias=d64.sum(dim=(0, 1)))
    yard = dict(mse=torch.stack([torch.mean(d32[t] ** 2) for t in range(steps)]), mae=torch.stack([torch.mean(d32[t].abs()) for t in range(steps)]),
                ray_sq_error=(d32 ** 2).reshape(-1, R).sum(dim=0), ray_abs_error=d32.abs().reshape(-1, R).sum(dim=0), ray_bias=d32.reshape(-1, R).sum(dim=0))
    for key in want:
        got = first[key][1].cpu().double()
        err = float(((got - want[key]).abs() / want[key].abs()).max())
        gap = float(((yard[key].double() - want[key]).abs() / want[key].abs()).max())
        bar = max(FLOOR, 4.0 * gap)
        print(f"{key}: kernel against float64 {err:.3e}, torch fp32 against float64 {gap:.3e}, bar {bar:.3e}")
        assert err <= bar, key
    amax = d32.abs().reshape(-1, R).amax(dim=0)
    print("ray_max_error equals amax:", torch.equal(first["ray_max_error"][1].cpu(), amax))
    assert torch.equal(first["ray_max_error"][1].cpu(), amax)


def test_python_wrapper_and_one_step_rows():
    """`rl.estimation_errors` on (n, R) rows of one step: the dict's shapes, and the first step WRITES the rows (nothing is read from them)."""
    from extended_legged_gym_amd.rl import estimation_errors
    g = torch.Generator(device="cuda").manual_seed(5)
    pred, tgt = torch.randn(7, 25, device="cuda", generator=g), torch.randn(7, 25, device="cuda", generator=g).abs()
    out = estimation_errors(pred, tgt)
    assert out["mse"].shape == (1,) and out["ray_bias"].shape == (25,)
    assert torch.equal(out["ray_max_error"], (pred - tgt).abs().amax(dim=0))
    assert float(out["mse"][0]) == pytest.approx(float(torch.mean((pred - tgt) ** 2)), rel=1e-5)
    with pytest.raises(ValueError, match="contiguous float32"):
        estimation_errors(pred.double(), tgt.double())

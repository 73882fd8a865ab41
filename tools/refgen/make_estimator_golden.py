"""Golden vectors of the terrain estimator -> tests/golden/terrain_estimator.npz, recorded from the reference's own `TerrainEstimator`
(`rsl_rl/modules/terrain_estimator.py`), imported through `ref_loader` and run on the CPU.

The full-size module has 603 519 parameters (2.4 MB), and six steps of eight 58 x 87 images are another megabyte: too large to commit.  So
the weights AND the depth images follow closed-form rules of the flat index (`closed_form_state`, `closed_form_depth` of
`tools/train_estimator.py`, which the tests call again), and the file holds only the small inputs (base velocities, resets), the expected
predictions and hidden states per step, and each case's own gap between the fp32 and the float64 module.

Cases: 28 x 56 GRU 256 (the default), 28 x 56 LSTM, 58 x 87 GRU, relu, tanh; each 6 consecutive steps of 8 rows, `reset(dones)` after steps
1 and 3 (`EstimatorDistillation.process_env_step`, `algorithms/distillation.py:275`)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402
from train_estimator import GOLDEN_CASES, closed_form_depth, closed_form_state  # noqa: E402

T, N, P, R = 6, 8, 6, 81


def run(case, dtype):
    from rsl_rl.modules.terrain_estimator import TerrainEstimator
    name, shape, mem, act = case
    with contextlib.redirect_stdout(io.StringIO()):
        est = TerrainEstimator(shape, P, R, memory_type=mem, activation=act)
    est.load_state_dict(closed_form_state(est, salt=GOLDEN_CASES.index(case)))
    est = est.to(dtype)
    depth = closed_form_depth(T, N, *shape).to(dtype)
    rng = np.random.default_rng(100 + GOLDEN_CASES.index(case))
    proprio = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(T, N, P)).astype(np.float32))
    dones = np.zeros((T, N), np.float32)
    dones[1, [0, 5]] = 1.0
    dones[3, [2, 5, 7]] = 1.0
    preds, hs = [], []
    with torch.no_grad():
        for t in range(T):
            preds.append(est.act_inference(depth[t], proprio[t].to(dtype)).clone())
            h = est.get_hidden_states()
            hs.append(torch.stack([x.clone() for x in (h if isinstance(h, tuple) else (h,))]))          # (1 or 2, L, N, H)
            est.reset(torch.from_numpy(dones[t]))
    return proprio.numpy(), dones, torch.stack(preds), torch.stack(hs)


def main():
    ref_loader.install_stubs()
    out = {}
    for case in GOLDEN_CASES:
        proprio, dones, p32, h32 = run(case, torch.float32)
        _, _, p64, h64 = run(case, torch.float64)
        name = case[0]
        out[name + "/proprio"], out[name + "/dones"] = proprio, dones
        out[name + "/predictions"], out[name + "/hidden"] = p32.numpy(), h32.numpy()
        out[name + "/gap"] = np.array([(p32.double() - p64).abs().max().item(), (h32.double() - h64).abs().max().item()])
        print(name, "pred |max|", float(p32.abs().max()), "gap", out[name + "/gap"])
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "terrain_estimator.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

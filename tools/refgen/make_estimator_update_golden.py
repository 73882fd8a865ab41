"""Golden figures for the native terrain-estimator update -> tests/golden/estimator_update.npz: the reference's vendored rsl_rl
(`EstimatorDistillation` + `EstimatorRolloutStorage`, `algorithms/distillation.py:190-433`, over `TerrainEstimator`) run in the build container on
torch-CPU, in the style of make_distillation_update_golden.py.  Weights and inputs are closed-form or seeded (tests/estimator_update_reference.Case),
so the file holds no weights and no rows: per case the returned loss, the per-step losses, the gradient norm of the last optimiser step, the
predictions on a probe batch (the rows of time index 1, from zero state) after the update, and the norm of every tensor of the post-update state --
each from the reference in float32 and again in float64 (the gap between the two is the e32 of the test's bar).

  gru_mse_clip   9 x 11, N 3, T 4, GRU, mse, G 3, E 1, max_grad_norm 1.0, lr 2e-3: one group and a one-step remainder
  lstm_huber     9 x 11, N 3, T 4, LSTM, huber, G 3, E 2, no clip, lr 2e-3: the second group wraps the epoch boundary, two remainder steps

Data only."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

sys.path.insert(0, ref_loader.REPO_ROOT)
from tests import estimator_update_reference as ref  # noqa: E402

CASES = {
    "gru_mse_clip": dict(case=dict(memory="gru", loss="mse", **ref.UPDATE_CASE), alg=dict(num_learning_epochs=1, gradient_length=3, learning_rate=2e-3, max_grad_norm=1.0)),
    "lstm_huber": dict(case=dict(memory="lstm", loss="huber", **ref.UPDATE_CASE), alg=dict(num_learning_epochs=2, gradient_length=3, learning_rate=2e-3, max_grad_norm=None)),
}


def run(spec, dtype):
    from rsl_rl.algorithms.distillation import EstimatorDistillation
    from rsl_rl.modules.terrain_estimator import TerrainEstimator
    case = ref.Case(**spec["case"])
    with contextlib.redirect_stdout(io.StringIO()):
        est = TerrainEstimator(case.shape, case.P, case.R, encoder_output_dim=case.F, memory_hidden_size=case.hidden, memory_num_layers=case.layers,
                               memory_type=case.memory, decoder_hidden_dims=list(case.decoder), activation=case.act)
    est.load_state_dict(ref.closed_form_state(est, case.salt))
    est = est.to(dtype)
    rows = ref.to_dtype(case.rows(), dtype)
    algo = EstimatorDistillation(est, loss_type=case.loss, device="cpu", **spec["alg"])
    algo.init_storage("distillation", case.N, case.T, list(case.shape), [case.P], [case.R])
    st = algo.storage
    st.depth_images, st.proprio_data, st.raycast_targets = rows["depth_images"].clone(), rows["proprio_data"].clone(), rows["raycast_targets"].clone()
    st.dones = st.dones.to(dtype)
    st.step = case.T
    losses, fn = [], algo.loss_fn

    def recording(pred, target):
        l = fn(pred, target)
        losses.append(l.item())
        return l
    algo.loss_fn = recording
    out = algo.update()
    est.reset()
    with torch.no_grad():
        probe = est.act_inference(rows["depth_images"][1], rows["proprio_data"][1])
    norms = np.array([float(v.double().norm()) for v in est.state_dict().values()])
    return dict(loss=np.float64(out["estimation"]), step_losses=np.array(losses, np.float64), grad_norm=np.float64(algo.last_grad_norm),
                probe=probe.double().numpy(), norms=norms, keys=list(est.state_dict()))


def main():
    ref_loader.install_stubs()
    sys.path.insert(0, os.path.join(ref_loader.REF_ROOT, "rsl_rl"))
    out = {}
    for name, spec in CASES.items():
        r32, r64 = run(spec, torch.float32), run(spec, torch.float64)
        assert r32["keys"] == list(ref.Case(**spec["case"]).state())
        for tag, r in (("f32", r32), ("f64", r64)):
            for k in ("loss", "step_losses", "grad_norm", "probe", "norms"):
                out[f"{name}.{tag}.{k}"] = r[k]
        print(name, "loss", r64["loss"], "f32 gap", abs(r32["loss"] - r64["loss"]) / r64["loss"], "steps", len(r64["step_losses"]), "grad norm", r64["grad_norm"])
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "estimator_update.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

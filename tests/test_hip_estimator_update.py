"""The native terrain-estimator update (include/lgestimator_train.h, `rl.NativeEstimatorDistillation`) on the GPU against
tests/estimator_update_reference.py in float64.

The bar is the one of tests/test_hip_ppo_update.py, measured and not guessed: torch's own fp32 CPU autograd on the same inputs deviates from float64
by e32(t) per tensor (e(t) = max|t - t64| / max|t64|); the kernels may deviate by at most max(8 e32(t), 2e-5).  Every figure is printed before it is
asserted.  tests/test_estimator_update_reference.py shows, without a GPU, that this bar sees the ways these kernels can go wrong."""
import pytest
import torch

from tests import estimator_update_reference as ref
from tests import ppo_reference as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slab():
    from extended_legged_gym_amd.rl.estimator_distillation import _estimator_train_lib
    return int(_estimator_train_lib().lg_estimator_train_wgrad_slab_rows())


def _estimator(case, state, precision="fp32"):
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    return NativeTerrainEstimator(state, case.shape, case.P, activation=case.act, memory_type=case.memory, device=DEV, encoder_precision=precision)


def _build(case, state=None, **kw):
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation
    state = state or case.state()
    est = _estimator(case, state)
    kw.setdefault("gradient_length", case.G)
    kw.setdefault("loss_type", case.loss)
    return est, NativeEstimatorDistillation(est, state, **kw)


def _cuda(rows):
    return {k: v.to(DEV) for k, v in rows.items()}


def _dev(state):
    return tuple(s.to(DEV) for s in state) if isinstance(state, tuple) else state.to(DEV)


def _within(name, e, e32):
    bar = ref.bar(e32)
    print(f"{name}: e {e:.3e}  e32 {e32:.3e}  e/e32 {e / max(e32, 1e-300):.2f}  bar {bar:.3e}")
    return e <= bar


def _rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def _state_err(got, want):
    return max(ref.err(g, w) for g, w in zip(ref._each(got), ref._each(want)))


# ------------------------------------------------------------------------------------------------------------ 1. one group against float64
def _group_cases():
    return ref.group_cases() + [ref.slab_case(8192)]


@pytest.mark.parametrize("case", _group_cases(), ids=lambda c: c.name)
def test_group_gradients_against_float64(case):
    """Every tensor's gradient, the global norm and each step loss within the bar; the trainer's predictions bit-equal to `act_inference` stepped over
    the same rows from the same state."""
    if case.name == "9x11_slabs":
        case = ref.slab_case(_slab())
    use_dones, carry, rows = bool(case.dones_at), ref.carry_of(case), case.rows()
    g64, n64, l64, p64, _ = ref.group_gradients(case, torch.float64, carry=carry, use_dones=use_dones)
    g32, n32, l32, _, _ = ref.group_gradients(case, torch.float32, carry=carry, use_dones=use_dones)
    assert all(float(g.abs().max()) > 0 for g in g64.values())
    est, alg = _build(case, use_dones=use_dones)
    alg.set_hidden_states(carry)
    alg.group(_cuda(rows), 0, case.G)
    grads, norm, losses = alg.gradients()
    preds = alg.forward_outputs().view(case.G, case.N, case.R)
    ok = True
    for k in g64:
        ok &= _within(f"{case.name} {k}", ref.err(grads[k], g64[k]), ref.err(g32[k], g64[k]))
    ok &= _within(f"{case.name} norm", _rel(norm, n64), _rel(n32, n64))
    for s in range(case.G):
        ok &= _within(f"{case.name} loss[{s}]", _rel(losses[s], l64[s]), _rel(l32[s], l64[s]))
    print(f"{case.name} predictions vs float64: {ref.err(preds, p64):.3e}")
    # the same rows through the inference kernels of a second estimator with the weights the group started from
    live = _estimator(case, case.state())
    live.set_hidden_states(_dev(carry))
    crows = _cuda(rows)
    for s in range(case.G):
        out = live.act_inference(crows["depth_images"][s], crows["proprio_data"][s])
        assert torch.equal(out.cpu(), preds[s]), f"step {s}: the trainer's forward is not act_inference's bit for bit"
        if use_dones:
            live.reset(crows["dones"][s])
    for part in (alg, est, live):
        part.close()
    assert ok


# ------------------------------------------------------------------------------------------------------------ 2. the optimiser step
def _ulp(t):
    t = t.double().abs()
    return torch.where(t > 0, 2.0 ** (torch.floor(torch.log2(t.clamp_min(1e-300))) - 23), torch.full_like(t, 2.0 ** -149))


@pytest.mark.parametrize("max_grad_norm", [ref.CLIP_SMALL, ref.CLIP_LARGE, None])
def test_optimiser_step_on_the_kernels_own_gradients(max_grad_norm):
    """`clip_and_adam` in float64 on the gradients the kernels produced, from loaded non-zero moments at step 7: parameters within 1e-5 lr + 1 ulp,
    moments within 1e-6 relative (the figures of tests/test_hip_ppo_update.py).  One clip that bites, one that does not, and no clip at all with a norm
    above the smaller clip: the result is the unclipped step."""
    case = ref.Case(**ref.OPT_CASE)
    lr, params = 2.5e-3, case.state()
    est, alg = _build(case, learning_rate=lr, max_grad_norm=max_grad_norm)
    g = torch.Generator().manual_seed(8)
    state = dict(parameters=params, exp_avg={k: 0.01 * torch.randn(v.shape, generator=g) for k, v in params.items()},
                 exp_avg_sq={k: 1e-4 * torch.rand(v.shape, generator=g) for k, v in params.items()}, step=7, learning_rate=lr)
    alg.load_optimizer_state(state)
    back = alg.optimizer_state()
    assert back["step"] == 7 and back["learning_rate"] == lr
    for k in params:
        assert torch.equal(back["exp_avg"][k], state["exp_avg"][k]) and torch.equal(back["parameters"][k], params[k]), k
        assert torch.equal(back["exp_avg_sq"][k], state["exp_avg_sq"][k]), k
    alg.group(_cuda(case.rows()), 0, case.G)
    grads, norm, _ = alg.gradients()
    print("norm", norm, "max_grad_norm", max_grad_norm)
    assert ref.CLIP_SMALL < norm < ref.CLIP_LARGE
    want, wstate = pref.clip_and_adam(params, grads, dict(exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"], step=7), lr,
                                      max_grad_norm if max_grad_norm else float("inf"))
    after = alg.optimizer_state()
    assert after["step"] == 8
    worst = 0.0
    for k in params:
        tol = 1e-5 * lr + _ulp(want[k])
        worst = max(worst, float(((after["parameters"][k].double() - want[k]).abs() / tol).max()))
        for moment in ("exp_avg", "exp_avg_sq"):
            assert float((after[moment][k].double() - wstate[moment][k]).abs().max()) <= 1e-6 * float(wstate[moment][k].abs().max()) + 1e-12, (moment, k)
    print("largest |theta - theta64| / (1e-5 lr + 1 ulp):", worst)
    alg.close(); est.close()
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ 3. a whole update
@pytest.mark.parametrize("memory,loss,clip", [("gru", "mse", 1.0), ("lstm", "huber", None)])
def test_whole_update_against_float64(memory, loss, clip):
    """E = 2, T = 4, G = 3: groups (0 1 2) and (3 0 1) -- the second across the epoch boundary --, remainder (2 3); then a second update from the
    carried state.  Step losses, the returned mean, last_grad_norm, the carry and the predictions on a probe batch after each update."""
    case = ref.Case(memory=memory, loss=loss, **ref.UPDATE_CASE)
    E, lr, rows = 2, 2e-3, case.rows()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        first = ref.run_update(case, dtype, E=E, lr=lr, max_grad_norm=clip)
        probe1 = ref.predict(first["model"], case, rows, t=1)
        second = ref.run_update(case, dtype, E=E, max_grad_norm=clip, carry=first["carry"], model=first["model"], optimizer=first["optimizer"])
        runs[dtype] = (first, probe1, second, ref.predict(second["model"], case, rows, t=1))
    est, alg = _build(case, num_learning_epochs=E, learning_rate=lr, max_grad_norm=clip)
    probe_env = _estimator(case, case.state())
    ok = True
    for u in (0, 2):
        out = alg.update(_cuda(rows))
        r64, r32 = runs[torch.float64][u], runs[torch.float32][u]
        assert alg.optimizer_steps == r64["steps"] == 2
        losses = alg.step_losses()
        for s in range(E * case.T):
            ok &= _within(f"update {u // 2} loss[{s}]", _rel(losses[s], r64["losses"][s]), _rel(r32["losses"][s], r64["losses"][s]))
        ok &= _within(f"update {u // 2} mean", _rel(out["estimation"], r64["mean"]), _rel(r32["mean"], r64["mean"]))
        ok &= _within(f"update {u // 2} last_grad_norm", _rel(alg.last_grad_norm, r64["grad_norm"]), _rel(r32["grad_norm"], r64["grad_norm"]))
        ok &= _within(f"update {u // 2} carry", _state_err(alg.get_hidden_states(), r64["carry"]), _state_err(r32["carry"], r64["carry"]))
        est.reset()
        got = est.act_inference(rows["depth_images"][1].to(DEV), rows["proprio_data"][1].to(DEV))
        ok &= _within(f"update {u // 2} probe predictions", ref.err(got, runs[torch.float64][u + 1]), ref.err(runs[torch.float32][u + 1], runs[torch.float64][u + 1]))
    assert alg.num_updates == 2
    for part in (alg, est, probe_env):
        part.close()
    assert ok


# ------------------------------------------------------------------------------------------------------------ 4. coherence and determinism
def _state_equal(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


def _states_equal(a, b):
    for x, y in zip(ref._each(a), ref._each(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("memory", ["gru", "lstm"])
def test_update_is_deterministic_equals_the_loop_of_groups_and_moves_the_live_estimator(memory):
    from tools.train_estimator import TerrainEstimatorTorch
    case = ref.Case(memory=memory, **ref.UPDATE_CASE)
    E, T, G, rows = 2, case.T, case.G, _cuda(case.rows())
    kw = dict(num_learning_epochs=E, learning_rate=4e-3, max_grad_norm=0.5, loss_type="huber")
    (est1, one), (est2, two), (est3, loop) = (_build(case, **kw) for _ in range(3))
    # the live inference state of the estimator is its own: an update neither reads nor writes it
    est1.act_inference(rows["depth_images"][0], rows["proprio_data"][0])
    live = tuple(s.clone() for s in ref._each(est1.get_hidden_states()))
    loss1, loss2 = one.update(rows), two.update(rows)
    _states_equal(live, est1.get_hidden_states())
    for first, n in ((0, G), (G, G)):
        loop.group(rows, first, n)
    loop.group(rows, 2 * G, E * T - 2 * G, train=False)
    loop.set_hidden_states(loop.get_hidden_states(running=True))
    assert loss1 == loss2
    assert torch.equal(one.step_losses(), two.step_losses())
    for other in (two, loop):
        _state_equal(one.optimizer_state(), other.optimizer_state())
        _states_equal(one.get_hidden_states(), other.get_hidden_states())
    # a second update from the carried state, again bit for bit
    assert one.update(rows) == two.update(rows)
    _state_equal(one.optimizer_state(), two.optimizer_state())
    _states_equal(one.get_hidden_states(), two.get_hidden_states())
    # the SAME estimator object acts as a fresh one built from the trained state dict does; a bf16 one loads it; the torch module loads it
    sd = one.state_dict()
    fresh, bf16 = _estimator(case, sd), _estimator(case, sd, precision="bf16")
    for e in (est1, fresh, bf16):
        e.reset()
    a = est1.act_inference(rows["depth_images"][2], rows["proprio_data"][2])
    b = fresh.act_inference(rows["depth_images"][2], rows["proprio_data"][2])
    c = bf16.act_inference(rows["depth_images"][2], rows["proprio_data"][2])
    assert torch.equal(a, b)
    assert torch.isfinite(c).all() and float((c - a).abs().max()) < 0.1 * float(a.abs().max())
    module = TerrainEstimatorTorch(case.shape, case.P, case.R, encoder_output_dim=case.F, memory_hidden_size=case.hidden, memory_num_layers=case.layers,
                                   memory_type=case.memory, decoder_hidden_dims=case.decoder, activation=case.act)
    module.load_state_dict(sd)
    back = module.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    for part in (one, two, loop, est1, est2, est3, fresh, bf16):
        part.close()


def test_carry_rules():
    """An update with another N than the carry's is refused until the carry is reset; the carry can be read and set."""
    case = ref.Case(**ref.UPDATE_CASE)
    est, alg = _build(case)
    assert alg.get_hidden_states() is None
    rows = _cuda(case.rows())
    alg.update(rows)
    h = alg.get_hidden_states()
    assert h.shape == (case.layers, case.N, case.hidden) and float(h.abs().max()) > 0
    fewer = {k: v[:, :2].contiguous() for k, v in rows.items()}
    with pytest.raises(Exception, match="lg_estimator_train_update: N is not the carry's"):
        alg.update(fewer)
    alg.set_hidden_states(None)
    alg.update(fewer)
    assert alg.get_hidden_states().shape == (case.layers, 2, case.hidden)
    alg.set_hidden_states(h)
    assert torch.equal(alg.get_hidden_states(), h)
    alg.close(); est.close()


# ------------------------------------------------------------------------------------------------------------ 5. the reference's own update
@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_update_against_the_references_own(name):
    """tests/golden/estimator_update.npz: the reference's `EstimatorDistillation` + `EstimatorRolloutStorage` + `TerrainEstimator` on torch-CPU, in
    float64 (what the update is held to) and in float32 (whose gap to float64 is the e32 of the bar)."""
    spec, gold = ref.GOLDEN_CASES[name], ref.golden(name)
    w64, w32 = gold["f64"], gold["f32"]
    case = ref.Case(**spec["case"])
    rows = case.rows()
    est, alg = _build(case, num_learning_epochs=spec["E"], learning_rate=spec["lr"], max_grad_norm=spec["max_grad_norm"])
    out = alg.update(_cuda(rows))
    losses = alg.step_losses()
    ok = True
    for s in range(len(w64["step_losses"])):
        ok &= _within(f"{name} loss[{s}]", _rel(losses[s], w64["step_losses"][s]), _rel(w32["step_losses"][s], w64["step_losses"][s]))
    ok &= _within(f"{name} returned loss", _rel(out["estimation"], w64["loss"]), _rel(w32["loss"], w64["loss"]))
    ok &= _within(f"{name} last_grad_norm", _rel(alg.last_grad_norm, w64["grad_norm"]), _rel(w32["grad_norm"], w64["grad_norm"]))
    est.reset()
    probe = est.act_inference(rows["depth_images"][1].to(DEV), rows["proprio_data"][1].to(DEV))
    ok &= _within(f"{name} probe predictions", ref.err(probe, torch.from_numpy(w64["probe"])), ref.err(torch.from_numpy(w32["probe"]), torch.from_numpy(w64["probe"])))
    sd = alg.state_dict()
    for k, n64, n32 in zip(sd, w64["norms"], w32["norms"]):
        ok &= _within(f"{name} |{k}|", _rel(sd[k].double().norm(), n64), _rel(n32, n64))
    alg.close(); est.close()
    assert ok


# ------------------------------------------------------------------------------------------------------------ 6. on collected rows
def test_three_updates_on_collected_rows():
    """`collect_estimation` on elspider_air_rough_raycast (small terrain), 64 envs, T = 6, G = 3, use_dones on the rows' real dones: three native
    updates against three float64 updates on the same rows -- returned losses, gradient norms, the carry and the predictions on a probe batch."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from train_estimator import make_env
    from extended_legged_gym_amd.rl import collect_estimation
    env = make_env(64, seed=3, small_terrain=True)
    env.reset()
    torch.manual_seed(11)
    with torch.inference_mode():
        batches = [{k: v.clone() for k, v in collect_estimation(env, None, 6).items()} for _ in range(3)]
    env.core.close()
    T, N, h, w = batches[0]["depth_images"].shape
    R = batches[0]["raycast_targets"].shape[2]
    case = ref.Case("collected", (h, w), N, 3, T=T, hidden=64, decoder=(32,), R=R, salt=12)
    cpu = [{k: v.cpu() for k, v in b.items()} for b in batches]
    runs = {}
    for dtype in (torch.float64, torch.float32):
        model = opt = carry = None
        trace = []
        for b in cpu:
            r = ref.run_update(case, dtype, lr=1e-3, use_dones=True, carry=carry, model=model, optimizer=opt, rows=b)
            model, opt, carry = r["model"], r["optimizer"], r["carry"]
            trace.append(r)
        runs[dtype] = (trace, ref.predict(model, case, cpu[0], t=2))
    est, alg = _build(case, learning_rate=1e-3, use_dones=True)
    ok = True
    for u, b in enumerate(batches):
        out = alg.update(b)
        r64, r32 = runs[torch.float64][0][u], runs[torch.float32][0][u]
        ok &= _within(f"update {u} mean", _rel(out["estimation"], r64["mean"]), _rel(r32["mean"], r64["mean"]))
        ok &= _within(f"update {u} last_grad_norm", _rel(alg.last_grad_norm, r64["grad_norm"]), _rel(r32["grad_norm"], r64["grad_norm"]))
        ok &= _within(f"update {u} carry", _state_err(alg.get_hidden_states(), r64["carry"]), _state_err(r32["carry"], r64["carry"]))
    est.reset()
    got = est.act_inference(batches[0]["depth_images"][2], batches[0]["proprio_data"][2])
    ok &= _within("probe predictions", ref.err(got, runs[torch.float64][1]), ref.err(runs[torch.float32][1], runs[torch.float64][1]))
    alg.close(); est.close()
    assert ok


# ------------------------------------------------------------------------------------------------------------ 7. the training tool
def test_train_tool_native_update_follows_the_torch_update():
    """`tools/train_estimator.py --update native` against `--update torch` (placed on the CPU, where it is reproducible): the actions are random, so
    both runs collect the same rows.  Iteration 0 runs both updates from the same weights: its loss (a mean of step losses, most of them taken before
    the first optimiser step) within the bar's 2e-5 floor.  Later iterations start from weights that two fp32 Adam histories produced -- a first step
    is +-lr whatever the gradient's size, so a gradient near zero may move a weight by 2 lr on one side only -- and are held to 1e-3."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from train_estimator import train
    kw = dict(steps=8, seed=4, gradient_length=4, log=lambda s: None, small_terrain=True)
    native = train(3, 32, update="native", **kw)
    eager = train(3, 32, update="torch", update_device="cpu", **kw)
    print("estimation loss, native update:", native, " torch update:", eager)
    assert len(native) == 3 and all(torch.isfinite(torch.tensor(native)))
    assert _rel(native[0], eager[0]) <= 2e-5
    assert all(_rel(a, b) <= 1e-3 for a, b in zip(native, eager))

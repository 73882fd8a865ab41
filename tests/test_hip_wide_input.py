"""GPU: networks whose input row is wider than one 512-column slab (`lg_mlp_create_wide`; csrc/lg_policy.hip: `mlp_wide_first_layer`) through
`lg_mlp_forward`, `lg_policy_act` and `lg_distill_act`, against float64 (`oracle.policy_oracle`).  Shapes: tests/wide_input.py; weights, rows, reference
and the bar max(2e-5, 4 x yardstick): tests/policy_sweep.py; the launch helpers (guarded buffers, the draw and log-prob checks) are those of
tests/test_hip_policy_sweep.py.  tests/test_wide_input_power.py (no GPU) shows on the same inputs that one layer-0 column read as zero, in any slab, moves
the output by thousands of bars.

Two properties of the split-K layer are held to equal bits: a network whose layer-0 weights are zero from column 512 on is the 512-input network
(every output keeps one k-ascending accumulator chain across the slabs), and a network whose only non-zero columns are the second slab's is the
narrow network on those columns (the result does not depend on where the slabs are cut)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import policy_oracle as po
from tests import policy_sweep as ps
from tests import wide_input as wi
from tests import test_hip_policy_sweep as sweep

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dims,act", wi.FORWARD_CASES, ids=[ps.case_id(d, a) for d, a in wi.FORWARD_CASES])
def test_forward_over_wide_shapes_rows_and_activations(dims, act):
    layers, x, want, yardstick, bar = ps.case(dims, act)
    mlp = sweep.native(layers, act)
    y70 = None
    for n in reversed(wi.ROWS):
        got = sweep.forward(mlp, x[:n].cuda(), f"{ps.case_id(dims, act)} n={n}")
        sweep.check_rows(f"{ps.case_id(dims, act)} n={n}", got, want[:n], bar, dims, yardstick)
        y70 = got if y70 is None else y70
        assert torch.equal(got, y70[:n]), f"{ps.case_id(dims, act)}: the first {n} rows depend on n"
    mlp.close()


@pytest.mark.parametrize("pair", range(len(wi.ACT_PAIRS)), ids=["x".join(str(n[0]) for n in p) for p in wi.ACT_PAIRS])
def test_act_kernels_with_wide_and_narrow_networks_in_one_launch(pair):
    adims, cdims = wi.ACT_PAIRS[pair]
    A, tdims, salt = adims[-1], ps.teacher_dims(cdims, adims[-1]), 20 + pair
    (al, ax, awant, ay, abar), (cl, cx, cwant, cy, cbar), (tl, tx, twant, ty, tbar) = (ps.case(d, "elu", salt=salt) for d in (adims, cdims, tdims))
    actor, critic, teacher = sweep.native(al), sweep.native(cl), sweep.native(tl)
    std = ps.std_vector(A).cuda()
    sdn = std.cpu().numpy()
    for n in wi.ROWS:
        obs, cobs = ax[:n].cuda(), cx[:n].cuda()
        fa, fc, ft = sweep.forward(actor, obs), sweep.forward(critic, cobs), sweep.forward(teacher, cobs)
        for call in wi.ACT_CALLS:
            tag = f"{adims} {cdims} n={n} call={call}"
            out = sweep.launch_policy_act(actor, critic, obs, cobs, std, call, 0, tag)
            sweep.check_rows(f"{tag} mean", out["mean"], awant[:n], abar, adims, ay)
            sweep.check_rows(f"{tag} values", out["values"], cwant[:n], cbar, cdims, cy)
            assert torch.equal(out["mean"], fa) and torch.equal(out["values"], fc), f"{tag}: lg_policy_act and lg_mlp_forward differ in bits"
            sweep.check_draw(tag, out["actions"], out["mean"], std, call)
            lp = po.normal_log_prob(out["actions"].cpu().numpy(), out["mean"].cpu().numpy(), sdn)
            np.testing.assert_allclose(out["logp"].cpu().numpy(), lp, rtol=1e-4, atol=1e-4)
            det = sweep.launch_policy_act(actor, critic, obs, cobs, std, call, 1, tag + " deterministic")
            assert torch.equal(det["actions"], fa) and torch.equal(det["values"], fc), tag
            dis = sweep.launch_distill_act(actor, teacher, obs, cobs, std, call, 0, tag + " distill")
            sweep.check_rows(f"{tag} distill mean", dis["mean"], awant[:n], abar, adims, ay)
            sweep.check_rows(f"{tag} teacher actions", dis["teacher_actions"], twant[:n], tbar, tdims, ty)
            assert torch.equal(dis["mean"], fa) and torch.equal(dis["teacher_actions"], ft), f"{tag}: lg_distill_act and lg_mlp_forward differ in bits"
            assert torch.equal(dis["actions"], out["actions"]), f"{tag}: lg_distill_act's draw is not lg_policy_act's"
    for m in (actor, critic, teacher):
        m.close()


def _extended(layers, K, first=0):
    """The same network reading rows of K columns: its layer-0 weights sit at columns first .. first + width, zeros elsewhere."""
    w0, b0 = layers[0]
    wide = np.zeros((w0.shape[0], K), np.float32)
    wide[:, first:first + w0.shape[1]] = w0
    return [(wide, b0)] + list(layers[1:])


@pytest.mark.parametrize("K", [513, 578, 1024, 1090])
def test_zero_weights_past_column_512_give_the_bits_of_the_512_input_network(K):
    al, _, _, _, _ = ps.case([512, 512, 32])
    cl, _, _, _, _ = ps.case([512, 33, 1], "elu", salt=30)
    x = ps.make_rows(K, salt=31)
    assert float(x[:, 512:].abs().max()) > 1.0          # the extra columns carry data: the zero weights must leave every chain as it is
    narrow_a, narrow_c = sweep.native(al), sweep.native(cl)
    wide_a, wide_c = sweep.native(_extended(al, K)), sweep.native(_extended(cl, K))
    std = ps.std_vector(32).cuda()
    for n in wi.ROWS:
        xw = x[:n].cuda()
        xn = xw[:, :512].contiguous()
        want = sweep.forward(narrow_a, xn)
        assert torch.equal(sweep.forward(wide_a, xw), want), (K, n)
        assert torch.equal(sweep.forward(wide_c, xw), sweep.forward(narrow_c, xn)), (K, n)
        a = sweep.launch_policy_act(narrow_a, narrow_c, xn, xn, std, 7, 0, f"narrow n={n}")
        for tag, critic, cobs in (("both wide", wide_c, xw), ("wide actor, narrow critic", narrow_c, xn)):
            b = sweep.launch_policy_act(wide_a, critic, xw, cobs, std, 7, 0, f"K={K} n={n} {tag}")
            assert all(torch.equal(a[k], b[k]) for k in a), (K, n, tag)
        b = sweep.launch_policy_act(narrow_a, wide_c, xn, xw, std, 7, 0, f"K={K} n={n} narrow actor, wide critic")
        assert all(torch.equal(a[k], b[k]) for k in a), (K, n)
    for m in (narrow_a, narrow_c, wide_a, wide_c):
        m.close()


def test_the_result_does_not_depend_on_where_the_slabs_are_cut():
    """640 inputs whose only non-zero layer-0 columns are 512 .. 639: the first slab adds exact zeros to every chain, the second slab IS the 128-input
    network's whole row."""
    for dims in ([128, 512, 1], [128, 16], [128, 65, 33, 7]):
        layers, _, _, _, _ = ps.case(dims)
        x = ps.make_rows(640, salt=32)
        narrow, wide = sweep.native(layers), sweep.native(_extended(layers, 640, first=512))
        for n in wi.ROWS:
            xw = x[:n].cuda()
            assert torch.equal(sweep.forward(wide, xw), sweep.forward(narrow, xw[:, 512:].contiguous())), (dims, n)
        narrow.close(); wide.close()


def test_a_578_wide_actor_critic_against_the_float64_module():
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeMLP
    adims, cdims = [578, 512, 256, 128, 18], [578, 512, 256, 128, 1]
    (al, x, awant, ay, abar), (cl, cx, cwant, cy, cbar) = ps.case(adims), ps.case(cdims, "elu", salt=33)
    sd = {}
    for prefix, layers in (("actor", al), ("critic", cl)):
        for j, (w, b) in enumerate(layers):
            sd[f"{prefix}.{2 * j}.weight"], sd[f"{prefix}.{2 * j}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    sd["std"] = ps.std_vector(18)
    policy = NativeActorCritic(sd, "elu", device="cuda:0", seed=ps.DRAW_SEED)
    assert policy.actor.dims[0] == 578 > abi.MLP_MAX_WIDTH
    obs, cobs = x.cuda(), cx.cuda()
    actions, values, logp, mean, sigma = policy.act_and_evaluate(obs, cobs)
    sweep.check_rows("act_and_evaluate mean", mean, awant, abar, adims, ay)
    sweep.check_rows("act_and_evaluate values", values, cwant, cbar, cdims, cy)
    sweep.check_draw("act_and_evaluate", actions, mean, policy.std, policy._call)
    lp = po.normal_log_prob(actions.cpu().numpy(), mean.cpu().numpy(), policy.std.cpu().numpy())
    np.testing.assert_allclose(logp.cpu().numpy(), lp, rtol=1e-4, atol=1e-4)
    sweep.check_rows("act_inference", policy.act_inference(obs), awant, abar, adims, ay)
    sweep.check_rows("evaluate", policy.evaluate(cobs), cwant, cbar, cdims, cy)
    with pytest.raises(RuntimeError, match=r"lg_mlp_create failed: lg_mlp_create: layer width out of range \(1\.\.512\)"):
        mlp = NativeMLP.__new__(NativeMLP)
        index = mlp._open("cuda:0")
        fp = C.POINTER(C.c_float)
        ws, bs = [w for w, _ in al], [b for _, b in al]
        mlp._created(mlp.lib.lg_mlp_create(4, (C.c_int32 * 5)(*adims), (fp * 4)(*[w.ctypes.data_as(fp) for w in ws]), (fp * 4)(*[b.ctypes.data_as(fp) for b in bs]),
                                           abi.ACTIVATIONS["elu"], index), "lg_mlp_create")

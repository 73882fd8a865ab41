"""CPU: can the sweep of the memory kernels (tests/test_hip_rnn_sweep.py, and the pass-edge cases R6 - R10 of tests/test_hip_ppo_recurrent_update.py) see
a fault?  No kernel runs here.

Forward: the float64 reference (`rnn_sweep.step`), on the sweep's own shapes, weights and inputs, is broken on purpose in the ways `rnn_tile`, `rnn_blocks`
and the host tiling (csrc/lg_rnn_tile.h, csrc/lg_policy.hip) can go wrong, and every fault must move some layer's h' or c' of the three steps by at least
POWER = 10 bars (bar = max(2e-5, 4 x the fp32-vs-float64 yardstick), the sweep's own rule).  These are conditions on the inputs: a weight set that fails
them gets another salt (`rnn_sweep.SALTS`), the factor stays.  A value "not read" is a zero in its place.  A position that does not exist at a layer
(k >= I, u >= H, no layer below layer 0) is no fault; a fault is left out only where the broken operation IS the true one -- the transposition of a
16-block fixes index 0, so a layer of one input, or of one state column, is exempt -- and what is left out is printed; at most a quarter of a case.

Backward: `ppo_recurrent_reference.cell` with `.detach()` on one operand, on the shapes whose gate derivative D has more than 1024 columns.  Every
fault must move at least one gradient tensor by ten of that tensor's own bars, max(8 e32, 2e-5)."""
import numpy as np
import pytest
import torch

from tests import ppo_recurrent_reference as rec
from tests import ppo_reference as pref
from tests import rnn_sweep as rs
from tests.test_hip_ppo_recurrent_update import ACT, GRAD_CASES, PASS_EDGE_SHAPES, SHAPES
from tests.test_hip_ppo_recurrent_update import _case as grad_case
from tests.test_policy_sweep_power import swap_accumulators, transpose_blocks, zero_col

POSITIONS = (0, 15, 16, -1)          # -1: the last column
PASS = 1024                          # BK_PASS of csrc/lg_train_recurrent.hip


def positions(width):
    return sorted({width - 1 if p < 0 else p for p in POSITIONS if p < width})


def without_bias(rnn, layers, l, slot, u):
    """The bias the tile adds to accumulator slot `slot` of unit u of layer l, zeroed: i f g o (b_ih + b_hh); r, z (b_ih + b_hh), n's b_in, n's b_hn."""
    H = layers[l][1].shape[1]
    out = [tuple(a.copy() for a in layer) for layer in layers]
    _, _, bi, bh = out[l]
    if rnn == "lstm" or slot < 2:
        bi[slot * H + u] = bh[slot * H + u] = 0.0
    elif slot == 2:
        bi[2 * H + u] = 0.0
    else:
        bh[2 * H + u] = 0.0
    return out


def swap_rows(h, c):
    return np.stack([swap_accumulators(a) for a in h]), (np.stack([swap_accumulators(a) for a in c]) if c is not None else None)


def row_31_from_32(x):
    x[31] = x[32]
    return x


def forward_faults(rnn, shape, layers):
    """([(name, layers to run, hooks)], [what was left out])."""
    I, H, L = shape
    out, left = [], []
    for l in range(L):
        K = I if l == 0 else H
        for k in positions(K):
            out.append((f"input column {k} of layer {l} read as zero", layers, dict(pre_x={l: zero_col(k)})))
        for u in positions(H):
            out.append((f"state column {u} of layer {l} read as zero", layers, dict(pre_h={l: zero_col(u)})))
            for slot, name in enumerate("ifgo" if rnn == "lstm" else ("r", "z", "n (b_in)", "n (b_hn)")):
                out.append((f"bias of unit {u} of gate {name} of layer {l} missing", without_bias(rnn, layers, l, slot, u), None))
        for width, key, what in ((K, "pre_x", "inputs"), (H, "pre_h", "state columns")):
            if width >= 2:
                out.append((f"{what} of layer {l} transposed within a 16-block", layers, {key: {l: transpose_blocks}}))
            else:
                left.append(f"{what} of layer {l} transposed within a 16-block: one column, index 0 is its own partner")
    out.append(("gates " + ("i and f" if rnn == "lstm" else "r and z") + " exchanged", layers, dict(swap_gates=True)))
    if rnn == "gru":
        out.append(("b_hn outside r * (...)", layers, dict(bhn_outside=True)))
        out.append(("the carry z * h takes the unmasked h of a reset row", layers, dict(carry_unmasked=True)))
    else:
        out.append(("c not zeroed on a reset row", layers, dict(keep_c=True)))
    if L >= 2:
        out.append(("a layer reads the old h of the layer below", layers, dict(stale_below=True)))
    out.append(("rows r and r + 16 of a tile exchanged", layers, dict(post=swap_rows)))
    out.append(("row 31 takes row 32's input", layers, dict(pre_x={0: row_31_from_32})))
    return out, left


@pytest.mark.parametrize("rnn,shape", rs.CASES, ids=[rs.case_id(r, s) for r, s in rs.CASES])
def test_every_forward_fault_moves_a_state_by_ten_bars(rnn, shape):
    layers, x, reset, want, yardstick, bar = rs.case(rnn, shape)
    x, reset, tag = x.numpy(), reset.numpy(), rs.case_id(rnn, shape)
    assert rs.deviation(rs.run(rnn, layers, x, reset, hooks={}), want) == 0.0          # the hooked step IS the reference when nothing is hooked
    assert bar == rs.FLOOR
    faults, left = forward_faults(rnn, shape, layers)
    for what in left:
        print(f"{tag} {what}: left out")
    worst = None
    for name, lay, hooks in faults:
        moved = rs.deviation(rs.run(rnn, lay, x, reset, hooks=hooks), want)
        print(f"{tag} {name}: moved {moved:.3e} = {moved / bar:.0f} bars (yardstick {yardstick:.3e}, bar {bar:.3e})")
        assert moved >= rs.POWER * bar, (tag, name, moved, bar)
        worst = min(worst or moved, moved)
    assert len(faults) >= 10 and len(left) <= len(faults) // 4, (len(faults), left)
    print(f"{tag}: {len(faults)} faults ({len(left)} left out), the weakest at {worst / bar:.0f} bars")


def test_the_shape_list_reaches_every_path_of_the_tiling():
    """What had never run under a reference: chunk counts 9 (wave 0 walks two chunks, the others one) and 17 beside 1, 2 and 32; both parities of the x
    blocks and of the h blocks, which a GRU walks apart; the image at its limit Kp = 1024, ragged and not; depths 1 to 4; H < 16."""
    tiles = [t for s in rs.SHAPES for t in rs.tiling(s)]
    assert {1, 2, 9, 17, 32} <= {t["nch"] for t in tiles}
    assert {t["nbx"] % 2 for t in tiles} == {0, 1} and {t["nbh"] % 2 for t in tiles} == {0, 1}
    assert {(t["nbx"] % 2, t["nbh"] % 2) for t in tiles} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(t["nbx"] == 1 and t["nbh"] == 1 for t in tiles) and any(t["nbx"] == 1 and t["nbh"] == 2 for t in tiles) and any(t["nbx"] == 2 and t["nbh"] == 1 for t in tiles)
    assert max(t["Kp"] for t in tiles) == rs.KMAX and (511, 511, 1) in rs.SHAPES and (512, 512, 1) in rs.SHAPES
    assert {s[2] for s in rs.SHAPES} == {1, 2, 3, 4} and max(s[2] for s in rs.SHAPES) == rs.MAX_LAYERS
    assert any(s[1] < 16 for s in rs.SHAPES) and any(s[1] < 16 and s[2] > 1 for s in rs.SHAPES)
    assert all(1 <= s[0] <= 512 and 1 <= s[1] <= 512 for s in rs.SHAPES)
    assert all((r, s) in rs.CASES for r in rs.TYPES for s in rs.SHAPES)
    assert rs.ROWS == (1, 31, 32, 33, 70) and rs.STEPS == 3
    m = rs.reset_mask().numpy()
    assert all(m[r] == 1 for r in (0, 31)) and all(rs.reset_mask(n).numpy()[-1] == 1 for n in rs.ROWS) and 0.2 <= m.mean() <= 0.4, m.mean()
    assert all(np.array_equal(rs.reset_mask(n).numpy(), m[:n]) for n in rs.ROWS)
    (a0, c0), (a1, c1) = rs.PAIRS
    assert a0[2] == c0[2] and a0[1] != c0[1] and a0[0] != c0[0] and a1[2] != c1[2]
    assert all(a in rs.SHAPES for a, _ in rs.PAIRS) and all(s in rs.SHAPES for s in rs.TRAIN_SHAPES)
    assert all(any(c[:2] == s[:2] for s in rs.SHAPES) and c[2] <= rs.MAX_LAYERS for _, c in rs.PAIRS)          # (33, 9) at the actor's depth 3
    d = rs.pair_dones().numpy()
    assert d[:, 0].any() and d[:, -1].any() and 0 < d.mean() < 0.5


def test_the_reference_is_torchs_lstm_and_gru():
    """`rnn_sweep.step` against `torch.nn.LSTM` / `nn.GRU` in float64 on one shape of each parity, with the reset as `Memory.reset(dones)` applies it."""
    for rnn, shape in (("lstm", (15, 17, 3)), ("gru", (15, 17, 3)), ("lstm", (33, 9, 2)), ("gru", (33, 9, 2))):
        layers, x, reset, want, _, _ = rs.case(rnn, shape)
        I, H, L = shape
        net = (torch.nn.LSTM if rnn == "lstm" else torch.nn.GRU)(I, H, L).double()
        net.load_state_dict({f"{name}_l{l}": torch.from_numpy(a).double() for l, layer in enumerate(layers)
                             for name, a in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), layer)})
        h = torch.zeros(L, rs.MAX_ROWS, H, dtype=torch.float64)
        st = (h, h.clone()) if rnn == "lstm" else h
        for t in range(rs.STEPS):
            if t == rs.RESET_STEP:
                for s in (st if rnn == "lstm" else (st,)):
                    s[:, reset == 1, :] = 0.0
            with torch.no_grad():
                _, st = net(x[t].double().unsqueeze(0), st)
            for got, ref in zip(st if rnn == "lstm" else (st,), want[t]):
                assert float(np.abs(got.numpy() - ref).max()) <= 1e-12, (rnn, shape, t)


def test_pair_and_training_policies_are_o1_under_the_floor():
    """The memories of the act pairs (critic at salt + 1) go through `case` too: yardstick under the floor, states O(1)."""
    for rnn in rs.TYPES:
        for a, c in rs.PAIRS:
            for shape, salt in ((a, 0), (c, 1)):
                _, _, _, _, yardstick, bar = rs.case(rnn, shape, salt=salt)
                print(f"{rs.case_id(rnn, shape)} salt {salt}: yardstick {yardstick:.3e}, bar {bar:.3e}")
                assert bar == rs.FLOOR
            sd = rs.policy_state(rnn, a, c)
            assert len(rs.memory_layers(sd, "memory_a")) == a[2] and len(rs.memory_layers(sd, "memory_c")) == c[2]
            assert np.array_equal(rs.memory_layers(sd, "memory_c")[0][0], rs.make_layers(rnn, c, 1)[0][0])


# ------------------------------------------------------------------------------------------------ the backward across its pass edges
def faulty_cell(fault):
    """`ppo_recurrent_reference.cell` with one operand detached: the values are the true ones, one path of the gradient is cut.
      a  columns >= 1024 of D do not reach dh_prev          b  only columns >= 1024 reach it (a second pass that overwrites)
      c  columns >= 1024 do not reach dx of a layer >= 1    d  a GRU's direct z dh term is dropped"""
    def cell(params, prefix, l, rnn_type, x, h, c):
        p = lambda name: params[f"{prefix}.rnn.{name}_l{l}"]          # noqa: E731
        lin = torch.nn.functional.linear
        wi, wh, bi, bh = p("weight_ih"), p("weight_hh"), p("bias_ih"), p("bias_hh")
        x_hi = x.detach() if fault == "c" and l > 0 else x
        h_lo, h_hi = (h.detach() if fault == "b" else h), (h.detach() if fault == "a" else h)
        gi = torch.cat([lin(x, wi[:PASS], bi[:PASS]), lin(x_hi, wi[PASS:], bi[PASS:])], dim=1)
        gh = torch.cat([lin(h_lo, wh[:PASS], bh[:PASS]), lin(h_hi, wh[PASS:], bh[PASS:])], dim=1)
        H = h.shape[-1]
        if rnn_type == "lstm":
            g = gi + gh
            i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
            c2 = f * c + i * gg
            return o * torch.tanh(c2), c2
        r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * (h.detach() if fault == "d" else h), None
    return cell


def backward_faults(rnn_type, layers):
    return ["a", "b"] + (["c"] if layers >= 2 else []) + (["d"] if rnn_type == "gru" else [])


NAMES = {"a": "columns >= 1024 of D do not reach dh_prev", "b": "only columns >= 1024 of D reach dh_prev", "c": "columns >= 1024 of D do not reach dx of layer 1",
         "d": "the GRU's direct z dh term is dropped"}


@pytest.mark.parametrize("shape", PASS_EDGE_SHAPES)
def test_every_backward_fault_moves_a_gradient_by_ten_bars(shape, monkeypatch):
    sd, ro, rnn_type, T, N, env0, count, _ = grad_case(shape)
    L, H = SHAPES[shape][1], SHAPES[shape][2]
    assert (4 if rnn_type == "lstm" else 3) * H > PASS
    hyper = dict(pref.HYPER, use_clipped_value_loss=True, entropy_coef=0.01, value_loss_coef=0.8)
    g64 = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float64)[0]
    g32 = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float32)[0]
    e32 = {k: float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64}
    bars = {k: max(8.0 * e32[k], 2e-5) for k in g64}
    print(f"{shape}: e32 at most {max(e32.values()):.3e}")
    monkeypatch.setattr(rec, "cell", faulty_cell(None))
    same = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float64)[0]
    assert max(float((same[k] - g64[k]).abs().max() / g64[k].abs().max()) for k in g64) <= 1e-12          # the split cell IS the cell when nothing is detached
    for fault in backward_faults(rnn_type, L):
        monkeypatch.setattr(rec, "cell", faulty_cell(fault))
        got = rec.gradients(sd, ACT, rnn_type, ro, env0, count, hyper, torch.float64)[0]
        moved = {k: float((got[k] - g64[k]).abs().max() / g64[k].abs().max()) / bars[k] for k in g64}
        k = max(moved, key=moved.get)
        print(f"{shape} ({fault}) {NAMES[fault]}: {moved[k]:.0f} bars on {k} (e32 {e32[k]:.3e}, bar {bars[k]:.3e})")
        assert moved[k] >= rs.POWER, (shape, fault, moved[k])


def test_the_new_gradient_cases_reach_the_pass_edges():
    """From the list itself: a GRU with two passes, second passes of 2, 4, 8 and 16 columns and of a whole gate, two layers across the edge; below the edge,
    9 chunks and H < 16 at depth 3."""
    shapes = {k: v for k, v in SHAPES.items() if k in {s for s, _ in GRAD_CASES}}
    K = {k: (4 if v[0] == "lstm" else 3) * v[2] for k, v in shapes.items()}
    assert set(PASS_EDGE_SHAPES) == {k for k in K if PASS < K[k] < 2 * PASS}
    assert {K[k] - PASS for k in PASS_EDGE_SHAPES} == {2, 4, 8, 16, 512}
    assert any(shapes[k][0] == "gru" and shapes[k][1] == 2 for k in PASS_EDGE_SHAPES) and any(shapes[k][0] == "lstm" and shapes[k][1] == 2 for k in PASS_EDGE_SHAPES)
    assert any((v[2] + 15) // 16 == 9 for v in shapes.values()) and any(v[2] < 16 and v[1] == 3 and v[4] == 1 for v in shapes.values())

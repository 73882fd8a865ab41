"""CPU: can the sweep of the policy kernels (tests/test_hip_policy_sweep.py) see a fault?  No kernel runs here: the float64 reference
(`oracle.policy_oracle.mlp_forward`), on the sweep's own shapes, weights and inputs (tests/policy_sweep.py), is broken on purpose in the ways `mlp_tile`,
its host tiling and `policy_act_body` (csrc/lg_policy.hip) can go wrong, and every fault must move the network's output by at least POWER = 10 bars
(bar = max(2e-5, 4 x the fp32-vs-float64 yardstick), the sweep's own rule; for the draw 2e-5 on z).  These are conditions on the inputs: an input or a
weight set that fails them is changed, the factor stays.

A value "not read" is a zero in its place.  A (fault, layer, position) triple is left out only by a rule stated with the fault: the position does not
exist at that layer (k >= K, j >= N, no hidden layer at L = 1, no row 16 at n = 1), or the broken operation IS the true one there (the transposition of
a 16-block fixes index 0, so a layer of one input is exempt; counter word a equals a >> 1 at a = 0, so a single action is exempt; dropping call_hi is
the identity below 2**32).  One more rule, for ReLU alone: a hidden unit that is zero on all 70 rows of the true network (a dead unit -- under the weight
rule, which the issue fixes, the rows of a deep ReLU network converge and about half the units of its late layers are dead) is exempt from the faults that
touch only that unit when the faulty output equals the true one exactly: zero in place of zero is the true operation.  Every layer must still keep a live
position, and the exempt triples are printed."""
import numpy as np
import pytest

from oracle import policy_oracle as po
from tests import policy_sweep as ps

K_POSITIONS = (0, 15, 16, 63, 64, -1)          # -1: K - 1
J_POSITIONS = (0, 15, 16, -1)                  # -1: N - 1


def forward(layers, x, act, pre=None, post=None, skip_act=(), act_last=False):
    """`po.mlp_forward` with hooks: pre[l](h) edits layer l's input, post[l](h) its output (after the activation); the activation is left out after the
    layers in `skip_act` and added after the last with `act_last`."""
    h = np.asarray(x, np.float64)
    for l, (w, b) in enumerate(layers):
        if pre and l in pre:
            h = pre[l](h.copy())
        h = h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if (l < len(layers) - 1 and l not in skip_act) or (l == len(layers) - 1 and act_last):
            h = po._ACT[act](h)
        if post and l in post:
            h = post[l](h.copy())
    return h


def zero_col(k):
    def go(h):
        h[:, k] = 0.0
        return h
    return go


def transpose_blocks(h):
    """Inputs 4 s + j and 4 j + s of every 16-block exchanged, in the zero-padded image the kernel reads: IMG's two low index fields swapped."""
    n, K = h.shape
    Kp = (K + 15) // 16 * 16
    img = np.zeros((n, Kp))
    img[:, :K] = h
    return img.reshape(n, Kp // 16, 4, 4).transpose(0, 1, 3, 2).reshape(n, Kp)[:, :K]


def swap_accumulators(y):
    """Rows r and r + 16 of every 32-row tile exchanged where both exist."""
    y = y.copy()
    for r in range(y.shape[0]):
        if r % 32 < 16 and r + 16 < y.shape[0]:
            y[[r, r + 16]] = y[[r + 16, r]]
    return y


def mlp_faults(dims, layers):
    """(name, hidden unit (layer, column) the fault is confined to or None, faulty forward from (x, act)).  Positions that do not exist at a layer are
    left out (see the module docstring)."""
    L, out = len(layers), []
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        for k in sorted({K - 1 if p < 0 else p for p in K_POSITIONS if p < K}):
            out.append((f"input column {k} of layer {l} read as zero", (l - 1, k) if l else None, lambda x, act, l=l, k=k: forward(layers, x, act, pre={l: zero_col(k)})))
        for j in sorted({N - 1 if p < 0 else p for p in J_POSITIONS if p < N}):
            out.append((f"output column {j} of layer {l} missing", (l, j) if l < L - 1 else None, lambda x, act, l=l, j=j: forward(layers, x, act, post={l: zero_col(j)})))
            nb = [(w, b.copy()) for w, b in layers]
            nb[l][1][j] = 0.0
            out.append((f"bias of column {j} of layer {l} missing", (l, j) if l < L - 1 else None, lambda x, act, nb=nb: forward(nb, x, act)))
        if K >= 2:          # with one input the transposition moves nothing: index 0 is its own partner
            out.append((f"inputs of layer {l} transposed within a 16-block", None, lambda x, act, l=l: forward(layers, x, act, pre={l: transpose_blocks})))
        if l < L - 1:
            out.append((f"activation left out after layer {l}", None, lambda x, act, l=l: forward(layers, x, act, skip_act=(l,))))
    out.append(("activation also after the last layer", None, lambda x, act: forward(layers, x, act, act_last=True)))
    out.append(("rows r and r + 16 of a tile exchanged", None, lambda x, act: swap_accumulators(forward(layers, x, act))))

    def row_31_from_32(x, act):
        x = np.asarray(x, np.float64).copy()
        x[31] = x[32]
        return forward(layers, x, act)
    out.append(("row 31 takes row 32's input", None, row_31_from_32))
    return out


@pytest.mark.parametrize("dims,act", ps.FORWARD_CASES, ids=[ps.case_id(d, a) for d, a in ps.FORWARD_CASES])
def test_every_fault_moves_the_output_by_ten_bars(dims, act):
    layers, x, want, yardstick, bar = ps.case(dims, act)
    x = x.numpy()
    assert float(np.abs(forward(layers, x, act) - want).max()) <= 1e-12        # the hooked forward IS the reference when nothing is hooked (BLAS summation order aside)
    hidden, h = [], np.asarray(x, np.float64)
    for w, b in layers[:-1]:
        h = po._ACT[act](h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64))
        hidden.append(h)
    worst, seen, exempt, live_layers = None, 0, 0, set()
    for name, unit, broken in mlp_faults(dims, layers):
        moved = float(np.abs(broken(x, act) - want).max())
        if act == "relu" and unit is not None and moved == 0.0 and not hidden[unit[0]][:, unit[1]].any():
            print(f"{ps.case_id(dims, act)} {name}: exempt, unit {unit} is zero on every row with and without the fault")
            exempt += 1
            continue
        if unit is not None:
            live_layers.add(unit[0])
        print(f"{ps.case_id(dims, act)} {name}: moved {moved:.3e} = {moved / bar:.0f} bars (yardstick {yardstick:.3e}, bar {bar:.3e})")
        assert moved >= ps.POWER * bar, (dims, act, name, moved, bar)
        worst = min(worst or moved, moved)
        seen += 1
    assert seen >= 6 and bar == ps.FLOOR and exempt <= seen // 4 and live_layers == set(range(len(layers) - 1)), (seen, exempt, live_layers)
    print(f"{ps.case_id(dims, act)}: {seen} faults ({exempt} exempt), the weakest at {worst / bar:.0f} bars")


def test_the_shape_list_reaches_every_path_of_the_tiling():
    """What the issue lists as never run: input widths 1, 63 / 64 / 65 and 512; hidden chunk counts 12 (waves 0-3 prefetch a next chunk, 4-7 re-read their
    own), 8 (no wave has a next chunk) and 32 (three next chunks per wave); last layers of 16 / 17 / 33 / 100 / 512 columns; L = 1 and L = 8."""
    firsts = {d[0] for d in ps.DIMS}
    assert {1, 63, 64, 65, 512} <= firsts
    hidden_chunks = {((w + 63) & ~63) // 16 for d in ps.DIMS for w in d[1:-1]}
    assert {4, 8, 12, 32} <= hidden_chunks, hidden_chunks
    lasts = {d[-1] for d in ps.DIMS}
    assert {1, 16, 17, 33, 100, 512} <= lasts
    assert {len(d) - 1 for d in ps.DIMS} >= {1, 2, 3, 8} and max(len(d) - 1 for d in ps.DIMS) == 8
    assert all(1 <= w <= 512 for d in ps.DIMS for w in d)
    for a in ps.ACTS[1:]:
        assert all((d, a) in ps.FORWARD_CASES for d in ps.EVERY_ACT_DIMS)
    assert all((d, "elu") in ps.FORWARD_CASES for d in ps.DIMS)
    assert sorted(a[-1] for a, _ in ps.ACT_PAIRS) == [1, 2, 7, 16, 17, 31, 32]
    assert all(c[-1] == 1 and len(c) != len(a) and c[0] != a[0] for a, c in ps.ACT_PAIRS)
    assert any(c >= 1 << 32 for c in ps.DRAW_CALLS) and set(ps.ACT_ROWS) == {1, 33, 70}


def test_act_pairs_have_o1_outputs_under_the_floor():
    """The networks of the act sweep go through `case` too: yardstick under the floor, outputs O(1)."""
    for salt, (adims, cdims) in enumerate(ps.ACT_PAIRS):
        for dims in (adims, cdims, ps.teacher_dims(cdims, adims[-1])):
            _, _, want, yardstick, bar = ps.case(dims, "elu", salt=10 + salt)
            print(f"{dims}: yardstick {yardstick:.3e}, bar {bar:.3e}, max |y| {float(np.abs(want).max()):.3f}")
            assert bar == ps.FLOOR


# ------------------------------------------------------------------------------------------------ the draw
def draw(seed, call, rows, num_actions, swap=False, word_a=False, drop_hi=False):
    """`po.policy_act_draw` restated with its three faults as switches."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    a = np.arange(num_actions, dtype=np.uint64)[None, :]
    hi = 0 if drop_hi else (call >> 32) & 0xFFFFFFFF
    c3 = (call & 0xFFFFFFFF) ^ ((hi * 0x9E3779B9) & 0xFFFFFFFF)
    o = po.philox4x32_10(r & np.uint64(0xFFFFFFFF), r >> np.uint64(32), a if word_a else a >> np.uint64(1), np.uint64(c3), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1 = np.maximum((o[0] >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0), np.float32(5.9604645e-8))
    u2 = (o[1] >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
    rad, ang = np.sqrt(np.float32(-2.0) * np.log(u1)), np.float32(6.28318530717958647692) * u2
    odd = ((np.arange(num_actions) & 1)[None, :] == 1) != swap
    return np.where(odd, rad * np.sin(ang), rad * np.cos(ang)).astype(np.float32)


@pytest.mark.parametrize("num_actions", sorted(a[-1] for a, _ in ps.ACT_PAIRS))
def test_every_fault_of_the_draw_moves_z_by_ten_bars(num_actions):
    for call in ps.DRAW_CALLS:
        for rows in ps.ACT_ROWS:
            want = po.policy_act_draw(ps.DRAW_SEED, call, rows, num_actions)
            assert want.dtype == np.float32 and want.shape == (rows, num_actions)
            assert np.array_equal(draw(ps.DRAW_SEED, call, rows, num_actions), want)
            faults = [("sin and cos exchanged", dict(swap=True))]
            if num_actions >= 2:          # a = 0 is its own a >> 1
                faults.append(("counter word a in place of a >> 1", dict(word_a=True)))
            if call >= 1 << 32:           # below 2**32 there is no high word to drop
                faults.append(("call_hi ignored", dict(drop_hi=True)))
            for name, kw in faults:
                moved = float(np.abs(draw(ps.DRAW_SEED, call, rows, num_actions, **kw).astype(np.float64) - want).max())
                print(f"A = {num_actions} call {call} rows {rows} {name}: moved {moved:.3e} = {moved / ps.DRAW_BAR:.0f} bars")
                assert moved >= ps.POWER * ps.DRAW_BAR, (num_actions, call, rows, name, moved)


def test_the_draw_has_the_moments_the_gpu_test_asserts():
    z = po.policy_act_draw(11, 1, 4096 + 13, 12).astype(np.float64)          # tests/test_hip_policy.py: seed 11, first call, 4109 rows, 12 actions
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(np.mean(z ** 3)) < 0.05 and abs(np.mean(z ** 4) - 3.0) < 0.15
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.05


def test_the_draw_is_a_pure_function_of_seed_call_row_and_action():
    a = po.policy_act_draw(ps.DRAW_SEED, 7, 33, 17)
    assert np.array_equal(po.policy_act_draw(ps.DRAW_SEED, 7, 70, 17)[:33], a)          # more rows: the first ones unchanged
    assert np.array_equal(po.policy_act_draw(ps.DRAW_SEED, 7, 33, 32)[:, :17], a)       # more actions likewise
    for c in (0, 7, 123456789):
        lo, hi = po.policy_act_draw(ps.DRAW_SEED, c, 33, 17), po.policy_act_draw(ps.DRAW_SEED, c + (1 << 32), 33, 17)
        assert float(np.abs(lo - hi).max()) >= ps.POWER * ps.DRAW_BAR and not np.array_equal(lo, hi)
    assert not np.array_equal(po.policy_act_draw(ps.DRAW_SEED, 8, 33, 17), a)
    assert not np.array_equal(po.policy_act_draw(ps.DRAW_SEED + (1 << 32), 7, 33, 17), a)  # the key's high word counts


# ------------------------------------------------------------------------------------------------ what else the GPU file leans on
def test_the_activation_grid_is_normal_and_crosses_both_switch_points():
    x = ps.activation_grid()
    assert x.dtype == np.float32 and len(x) % 16 == 0 and np.all(np.isfinite(x))
    assert np.all((x == 0) | (np.abs(x) >= np.finfo(np.float32).tiny)) and float(np.abs(x).max()) == np.float32(30.0)
    q = np.float32(-0.25)
    assert {np.nextafter(q, np.float32(-1)), q, np.nextafter(q, np.float32(0))} <= set(x.tolist())
    assert {np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, 0.0} <= set(x.tolist())
    assert int(((x > -0.3) & (x < 0.05)).sum()) >= 4000
    for act in ("elu", "tanh", "selu"):
        _, yardstick, bar = ps.activation_reference(act, x)
        print(f"{act}: torch fp32 on the CPU is {yardstick:.3e} from float64 on the grid; bar {bar:.3e}")
        assert 2.0 ** -22 <= bar < 1e-5          # (selu: half an ulp of 1.05 x 30 is 1.9e-6)


def test_gae_inputs_reach_the_cases_the_issue_names():
    assert any(n % 256 for _, n in ps.GAE_SHAPES) and any(T * n < 1024 for T, n in ps.GAE_SHAPES) and any(T == 1 for T, _ in ps.GAE_SHAPES)
    assert any(n > 1024 for _, n in ps.GAE_SHAPES)
    for T, n in ps.GAE_SHAPES:
        r, d, v, last = ps.gae_inputs(T, n, "last")
        assert float(d[-1].min()) == 1.0 and float(d[:-1].sum()) == 0.0
        d = ps.gae_inputs(T, n, "random")[1]
        assert set(d.unique().tolist()) <= {0.0, 1.0}
        # a done on the last step cuts the bootstrap: the reference's last return is then reward alone
        ret, _ = po.compute_returns(r.numpy(), ps.gae_inputs(T, n, "last")[1].numpy(), v.numpy(), last.numpy(), 0.99, 0.95, False)
        np.testing.assert_allclose(ret[-1], r[-1].numpy().astype(np.float64), rtol=0, atol=1e-12)

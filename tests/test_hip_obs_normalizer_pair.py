"""`lg_obsnorm_step_pair` (include/lgrunner_privileged.h) through `NativeEmpiricalNormalization.step_pair`: one call over two handles against the two
single calls (`lg_obsnorm_step`), bit for bit in the outputs, in `_mean` / `_var` / `_std` / `count` and in the carried-row flags.  Row counts on
both sides of the slab and row-block sizes (1, 37, 64, 1000: one slab of one row, a ragged last slab, exactly 16 slabs of 4 rows, 125 slabs of
8); widths on both sides of a 64-column tile, with the two handles needing different numbers of tiles ((48, 235): 1 and 4; (144, 235): 3 and 4;
(65, 130): 2 and 3)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(n, oa, oc) for n in (1, 37, 64, 1000) for oa, oc in ((1, 1), (48, 235), (144, 235), (65, 130))]


def rows(n, width, seed, pad=0):
    """(n, width) rows with a per-column offset and scale, as a view of a (n, width + pad) buffer."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, width + pad, generator=g) * torch.linspace(0.1, 30.0, width + pad) + torch.linspace(-50.0, 50.0, width + pad)
    return buf.cuda()[:, :width]


def handles(oa, oc, until_a=None, until_c=None):
    from extended_legged_gym_amd.rl import NativeEmpiricalNormalization
    return NativeEmpiricalNormalization([oa], until=until_a, device="cuda:0"), NativeEmpiricalNormalization([oc], until=until_c, device="cuda:0")


def same_state(x, y, n):
    sx, sy = x.get_state(), y.get_state()
    assert sx[3] == sy[3], (sx[3], sy[3])
    for name, p, q in zip(("_mean", "_var", "_std"), sx[:3], sy[:3]):
        assert np.array_equal(p, q), (name, float(np.abs(p - q).max()))
    assert x.carried_row(n) is None and y.carried_row(n) is None          # a step never touches the carried row
    return sx[3]


def both_ways(single, pair, xa, xc, inplace):
    """One step on each pair of handles over equal copies of the rows; compares outputs and states; returns the two counts."""
    n = xa.shape[0]
    if inplace:
        sa, sc, pa, pc = xa.clone(), xc.clone(), xa.clone(), xc.clone()
        assert single[0].normalize_(sa) is sa and single[1].normalize_(sc) is sc
        ra, rc = pair[0].step_pair(pair[1], pa, pc, inplace=True)
        assert ra is pa and rc is pc
        want, got = (sa, sc), (pa, pc)
    else:
        keep = xa.clone(), xc.clone()
        want = single[0](xa), single[1](xc)
        got = pair[0].step_pair(pair[1], xa, xc)
        assert torch.equal(xa, keep[0]) and torch.equal(xc, keep[1])          # out of place: the inputs stay
    for w, g, side in zip(want, got, "ac"):
        assert w.shape == g.shape and torch.equal(w, g), (side, float((w - g).abs().max()))
    return same_state(single[0], pair[0], n), same_state(single[1], pair[1], n)


@pytest.mark.parametrize("n,oa,oc", SHAPES)
def test_pair_is_two_single_steps(n, oa, oc):
    for inplace in (False, True):
        single, pair = handles(oa, oc), handles(oa, oc)
        # two updating calls (the second on a non-initial count), then update off
        for k in range(2):
            counts = both_ways(single, pair, rows(n, oa, 10 * k + 1), rows(n, oc, 10 * k + 2), inplace)
            assert counts == ((k + 1) * n, (k + 1) * n)
        for h in single + pair:
            h.eval()
        before = pair[0].get_state(), pair[1].get_state()
        assert both_ways(single, pair, rows(n, oa, 31), rows(n, oc, 32), inplace) == (2 * n, 2 * n)
        for b, h in zip(before, pair):
            assert all(np.array_equal(p, q) for p, q in zip(b[:3], h.get_state()[:3]))


@pytest.mark.parametrize("n,oa,oc", SHAPES)
@pytest.mark.parametrize("frozen", ["actor", "critic"])
def test_one_handle_frozen_while_the_other_counts(n, oa, oc, frozen):
    until = dict(until_a=n) if frozen == "actor" else dict(until_c=n)          # frozen from the second call on
    single, pair = handles(oa, oc, **until), handles(oa, oc, **until)
    for k in range(3):
        ca, cc = both_ways(single, pair, rows(n, oa, 5 * k + 1), rows(n, oc, 5 * k + 2), inplace=bool(k % 2))
        live, held = (k + 1) * n, n
        assert (ca, cc) == ((held, live) if frozen == "actor" else (live, held))


@pytest.mark.parametrize("n,oa,oc", [s for s in SHAPES if s[0] > 1])
@pytest.mark.parametrize("side", ["actor", "critic"])
def test_row_stride_on_one_side_only(n, oa, oc, side):
    """Rows of a wider buffer (row_stride > O) on one side, contiguous rows on the other; in place the columns past O stay untouched."""
    single, pair = handles(oa, oc), handles(oa, oc)
    for k in range(2):
        xa, xc = rows(n, oa, 7 * k + 1, pad=5 if side == "actor" else 0), rows(n, oc, 7 * k + 2, pad=3 if side == "critic" else 0)
        assert (xa.stride(0) > oa) == (side == "actor") and (xc.stride(0) > oc) == (side == "critic")
        both_ways(single, pair, xa, xc, inplace=False)
    wide = rows(n, oa + 5, 99) if side == "actor" else rows(n, oc + 3, 99)
    keep = wide.clone()
    xa, xc = (wide[:, :oa], rows(n, oc, 98)) if side == "actor" else (rows(n, oa, 98), wide[:, :oc])
    pair[0].step_pair(pair[1], xa, xc, inplace=True)
    width = oa if side == "actor" else oc
    assert torch.equal(wide[:, width:], keep[:, width:]) and not torch.equal(wide[:, :width], keep[:, :width])


def test_refusals_carry_their_reason():
    a, c = handles(48, 235)
    with pytest.raises(ValueError, match="rows"):
        a.step_pair(c, rows(4, 48, 1), rows(5, 235, 2))
    with pytest.raises(ValueError, match="235"):
        a.step_pair(c, rows(4, 48, 1), rows(4, 48, 2))
    c.eval()
    with pytest.raises(ValueError, match="modes"):
        a.step_pair(c, rows(4, 48, 1), rows(4, 235, 2))
    c.train()
    with pytest.raises(RuntimeError, match="lg_obsnorm_step_pair: one normaliser given twice"):
        a.step_pair(a, rows(4, 48, 1), rows(4, 48, 2))
    assert a.get_state()[3] == 0 and c.get_state()[3] == 0
    empty = a.step_pair(c, rows(0, 48, 1), rows(0, 235, 2))          # n = 0: nothing happens
    assert empty[0].shape == (0, 48) and empty[1].shape == (0, 235) and a.get_state()[3] == 0

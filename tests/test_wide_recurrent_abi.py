"""CPU side of the wide memory (include/lgpolicy_wide_memory.h, included by lgpolicy_wide.h: `lg_rnn_create_wide`, `LG_RNN_MAX_INPUT`,
`lg_rnn_tile_weights_wide`): the header, `abi.py` and the built library agree, the refusals start with the entry point's own name and name the
width that is wrong, `lg_rnn_create` keeps its own limit and message, the host tiling of the two images of a wide layer 0 is a pure, invertible
function, and the new memory kernels report no scratch, no spills and an LDS size a gfx950 workgroup can have while `rnn_layer_kernel` keeps its
128 KB.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, header_source, kernel_metadata, last_error, library

WIDE_MEMORY = ["lg_rnn_create_wide", "lg_rnn_tile_weights_wide"]          # what include/lgpolicy_wide_memory.h declares


def _lib():
    return library("policy", "policy_wide")


def test_header_abi_and_library_agree():
    hdr, wide_hdr, narrow_hdr = header_source("lgpolicy_wide_memory.h"), header_source("lgpolicy_wide.h"), header_source("lgpolicy.h")
    assert '#include "lgpolicy_wide_memory.h"' in wide_hdr                  # one include gives both wide create functions
    declared = set(re.findall(r"\b(lg_[a-z0-9_]+)\s*\(", hdr)) - set(abi.POLICY_SYMBOLS)
    assert sorted(declared) == WIDE_MEMORY and set(WIDE_MEMORY) < set(abi.symbols("policy_wide"))
    # lgpolicy_wide.h keeps to one symbol of its own: the unit is that one and the memory's two
    own = set(re.findall(r"\b(lg_[a-z0-9_]+)\s*\(", wide_hdr)) - set(abi.POLICY_SYMBOLS)
    assert own == {"lg_mlp_create_wide"} and sorted(own | declared) == sorted(abi.symbols("policy_wide"))
    assert int(re.search(r"#define\s+LG_RNN_MAX_INPUT\s+(\d+)", hdr).group(1)) == abi.RNN_MAX_INPUT == 2048
    assert abi.RNN_MAX_WIDTH == 512 and abi.RNN_MAX_INPUT % abi.RNN_MAX_WIDTH == 0
    proto = re.search(r"lg_rnn\*\s+lg_rnn_create_wide\(([^)]*)\)", hdr).group(1)
    narrow = re.search(r"lg_rnn\*\s+lg_rnn_create\(([^)]*)\)", narrow_hdr).group(1)
    assert re.sub(r"\s+", " ", proto) == re.sub(r"\s+", " ", narrow)          # the arguments of lg_rnn_create
    lib = _lib()
    for sym in WIDE_MEMORY:
        assert hasattr(lib, sym) and getattr(lib, sym).argtypes, sym
    assert lib.lg_rnn_create_wide.argtypes == lib.lg_rnn_create.argtypes and lib.lg_rnn_create_wide.restype is C.c_void_p


def _lists(null=False):
    fp = C.POINTER(C.c_float)
    w = np.zeros(16, np.float32)          # never read: every refusal below comes before the weights are touched
    return [None if null else (fp * 5)(*[w.ctypes.data_as(fp)] * 5) for _ in range(4)]


@pytest.mark.parametrize("args,words", [((0, 1, 0, 64), ("input", "1..2048")), ((0, 1, 2049, 64), ("input", "1..2048")), ((1, 1, 578, 513), ("hidden", "1..512")),
                                        ((0, 0, 578, 64), ("layers", "1..4")), ((1, 5, 578, 64), ("layers", "1..4")), ((7, 1, 578, 64), ("type",))])
def test_refusals_name_the_entry_point_and_the_width(args, words):
    lib = _lib()
    assert not lib.lg_rnn_create_wide(*args, *_lists(), 0), args
    msg = last_error(lib)
    assert msg.startswith("lg_rnn_create_wide: "), msg
    for word in words:
        assert word in msg, (args, msg)


def test_null_lists_are_refused():
    lib = _lib()
    assert not lib.lg_rnn_create_wide(0, 1, 578, 64, *_lists(null=True), 0)
    msg = last_error(lib)
    assert msg.startswith("lg_rnn_create_wide: ") and "null" in msg, msg


def test_the_diagnostic_switch_is_checked(monkeypatch):
    lib = _lib()
    monkeypatch.setenv("LG_RNN_FORCE_WIDE", "yes")
    assert not lib.lg_rnn_create_wide(0, 1, 578, 64, *_lists(), 0)
    msg = last_error(lib)
    assert msg.startswith("lg_rnn_create_wide: ") and "LG_RNN_FORCE_WIDE" in msg and "yes" in msg, msg


def test_the_narrow_entry_point_keeps_its_limit_and_message():
    lib = _lib()
    for I in (513, 578, 2048):
        assert not lib.lg_rnn_create(1, 1, I, 64, *_lists(), 0)
        msg = last_error(lib)
        assert msg == "lg_rnn_create: input width out of range (1..512)", (I, msg)
    assert lib.lg_rnn_tile_weights(0, 513, 64, None, None, None) < 0          # the one-image tiling stays at 512 too


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
@pytest.mark.parametrize("I", [513, 578, 1041, 2048])
@pytest.mark.parametrize("H", [1, 40, 512])
def test_wide_weight_tiling_round_trips(rnn_type, I, H):
    """`lg_rnn_tile_weights_wide` against the layout the header documents, inverted here in numpy: every weight comes back, everything else in the
    two images (padding rows / columns, the zero block that ends each chunk) is zero."""
    lib = _lib()
    G = 4 if rnn_type == "lstm" else 3
    rng = np.random.default_rng(I * 1000 + H)
    w_ih, w_hh = rng.normal(size=(G * H, I)).astype(np.float32), rng.normal(size=(G * H, H)).astype(np.float32)
    t = abi.RNN_TYPES[rnn_type]
    count_h = C.c_int64(0)
    count_x = lib.lg_rnn_tile_weights_wide(t, I, H, None, None, None, None, C.byref(count_h))
    nbx, nch = (I + 15) // 16, (H + 15) // 16
    assert count_x == nch * (nbx + 1) * G * 64 * 4 and count_h.value == nch * (nch + 1) * G * 64 * 4
    tx, th = np.full(count_x, np.nan, np.float32), np.full(count_h.value, np.nan, np.float32)
    assert lib.lg_rnn_tile_weights_wide(t, I, H, w_ih.ctypes.data, w_hh.ctypes.data, tx.ctypes.data, th.ctypes.data, None) == count_x
    lane = np.arange(64)
    for tiled, nb, want, K in ((tx, nbx, w_ih, I), (th, nch, w_hh, H)):
        tl = tiled.reshape(nch, nb + 1, G, 64, 4)
        # tl[c, b, g, lane, s] = W[g H + 16 c + (lane & 15)][16 b + 4 s + (lane >> 4)]
        w = np.zeros((G, 16 * nch, (nb + 1) * 16), np.float32)
        for c in range(nch):
            for b in range(nb + 1):
                for s in range(4):
                    w[:, 16 * c + (lane & 15), 16 * b + 4 * s + (lane >> 4)] = tl[c, b, :, :, s]
        np.testing.assert_array_equal(w[:, :H, :K].reshape(G * H, K), want)
        rest = w.copy()
        rest[:, :H, :K] = 0
        assert not rest.any() and np.isfinite(tiled).all()
    assert lib.lg_rnn_tile_weights_wide(t, 2049, H, None, None, None, None, None) < 0
    assert last_error(lib).startswith("lg_rnn_tile_weights_wide: ")
    assert lib.lg_rnn_tile_weights_wide(t, I, 513, None, None, None, None, None) < 0 and lib.lg_rnn_tile_weights_wide(5, I, H, None, None, None, None, None) < 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("source,new,kept", [("lg_policy.hip", ("rnn_wide_xproj_kernel", "rnn_wide_layer_kernel"), "rnn_layer_kernel"),
                                             ("lg_train_recurrent.hip", ("rnn_wide_train_forward_kernel",), "rnn_train_forward_kernel")])
def test_wide_memory_kernels_use_no_scratch_no_spills_and_fit_the_lds(source, new, kept):
    blocks = kernel_metadata(source)
    rnn = {k: v for k, v in blocks.items() if "rnn_" in k}
    for name in new + (kept,):
        assert len([k for k in rnn if name in k]) == 1, (name, sorted(blocks))          # (no new name contains an old one)
    for name, r in rnn.items():
        print(name, r)
        assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0, (name, r)          # the bar of tests/test_policy_recurrent_abi.py
        assert r["group_segment_fixed_size"] <= 160 * 1024, (name, r)
    for name in new:                     # one slab of 32 rows x 512 floats: two workgroups per CU, two waves per SIMD; and no scalar register parked in a
        r = [v for k, v in rnn.items() if name in k][0]          # vector lane either (rnn_layer_kernel has always parked 4; it is left as it is)
        assert r["group_segment_fixed_size"] == 32 * 512 * 4 and r["vgpr_count"] <= 256 and r.get("sgpr_spill_count", 0) == 0, (name, r)
    narrow = [v for k, v in rnn.items() if kept in k][0]
    assert narrow["group_segment_fixed_size"] == 32 * 1024 * 4 and narrow["vgpr_count"] <= 256, narrow

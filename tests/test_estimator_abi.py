"""CPU side of the terrain estimator (include/lgpolicy.h, section "terrain estimator"): the header names, the library's exports and the ctypes
mirror agree; `lg_conv_tile_weights` (a pure host function) against a numpy restatement of the documented layout for the four conv shapes and a
linear one, and its error returns; what is refused before any device is touched; the new kernels' code-object metadata (cross-compiled for
gfx950): no spills, no scratch, LDS within one workgroup's share of a compute unit.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, header_source, kernel, kernel_metadata, last_error, library

NEW = ["lg_conv_encoder_create", "lg_conv_encoder_destroy", "lg_conv_tile_weights", "lg_conv_encoder_forward", "lg_mlp_set_output_activation",
       "lg_estimator_step", "lg_conv_encoder_stage_shape", "lg_conv_encoder_forward_stages"]


def _lib():
    return library("policy")


def test_new_symbols_are_in_the_header_exported_and_declared():
    header = header_source("lgpolicy.h")
    lib = _lib()
    for sym in NEW:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in abi.POLICY_SYMBOLS and hasattr(lib, sym), sym
    assert "terrain_estimator.py:80-109" in header and "terrain_estimator.py:162-198" in header
    for sym in NEW:
        assert getattr(lib, sym).argtypes, sym
    from extended_legged_gym_amd import rl
    for name in ("NativeTerrainEstimator", "NativeConvEncoder", "collect_estimation", "parse_estimator_state"):
        assert hasattr(rl, name), name


def _tile_numpy(w):
    """The layout documented at lg_conv_tile_weights, restated."""
    cout, cin, kh, kw = w.shape
    K = cin * kh * kw
    nkb, nch = -(-K // 64) * 4, -(-cout // 64) * 4
    wk = np.zeros((nch * 16, nkb * 16), np.float32)
    wk[:cout, :K] = w.transpose(0, 2, 3, 1).reshape(cout, K)          # k = (ky kw + kx) c_in + ci
    lane, s = np.arange(64)[:, None], np.arange(4)[None, :]
    out = np.empty((nch, nkb, 64, 4), np.float32)
    for c in range(nch):
        for b in range(nkb):
            out[c, b] = wk[16 * c + (lane & 15), 16 * b + 4 * s + (lane >> 4)]
    return out.reshape(-1)


@pytest.mark.parametrize("shape", [(32, 1, 5, 5), (64, 32, 3, 3), (128, 64, 3, 3), (64, 128, 3, 3), (128, 1024, 1, 1), (70, 128, 1, 1)])
def test_conv_tile_weights_matches_the_documented_layout(shape):
    lib = _lib()
    rng = np.random.default_rng(sum(shape))
    w = rng.standard_normal(shape).astype(np.float32)
    count = lib.lg_conv_tile_weights(*shape, None, None)
    want = _tile_numpy(w)
    assert count == want.size
    tiled = np.full(count, np.nan, np.float32)
    assert lib.lg_conv_tile_weights(*shape, w.ctypes.data, tiled.ctypes.data) == count
    assert np.array_equal(tiled, want)
    assert np.count_nonzero(tiled) == np.count_nonzero(w)           # every weight exactly once, zeros elsewhere


def test_conv_tile_weights_error_returns():
    lib = _lib()
    buf = np.zeros(64 * 64 * 4, np.float32)
    for bad in ((0, 1, 3, 3), (513, 1, 3, 3), (32, 0, 3, 3), (32, 1025, 3, 3), (32, 1, 0, 3), (32, 1, 3, 16)):
        assert lib.lg_conv_tile_weights(*bad, None, None) == abi.LG_ERR_INVALID, bad
    assert lib.lg_conv_tile_weights(32, 1, 5, 5, None, buf.ctypes.data) == abi.LG_ERR_INVALID       # output asked for, no weights given


def test_refusals_that_need_no_device():
    lib = _lib()
    fp = C.POINTER(C.c_float)
    arrs = [np.zeros(4, np.float32) for _ in range(6)]
    lists = (fp * 6)(*[a.ctypes.data_as(fp) for a in arrs])         # never read: the sizes are refused first
    for args, word in (((129, 56, 64, 0), "image size"), ((28, 7, 64, 0), "image size"), ((28, 56, 513, 0), "out_dim"), ((28, 56, 0, 0), "out_dim"),
                       ((28, 56, 64, 3), "activation")):
        assert not lib.lg_conv_encoder_create(*args, lists, lists, 0), args
        msg = last_error(lib)
        assert "lg_conv_encoder_create" in msg and word in msg, (args, msg)
    assert not lib.lg_conv_encoder_create(28, 56, 64, 0, None, lists, 0)
    assert "null" in last_error(lib)
    p = 0x1000
    assert lib.lg_conv_encoder_forward(None, p, 1568, 4, p, None) == abi.LG_ERR_INVALID
    assert "lg_conv_encoder_forward" in last_error(lib)
    for stages in (1, 7, 0, 8):
        assert lib.lg_conv_encoder_forward_stages(None, p, 1568, 4, stages, p, None) == abi.LG_ERR_INVALID
        assert "lg_conv_encoder_forward_stages" in last_error(lib)
    assert lib.lg_conv_encoder_stage_shape(None, 1, None, None, None) == abi.LG_ERR_INVALID
    assert "lg_conv_encoder_stage_shape" in last_error(lib)
    assert lib.lg_estimator_step(None, None, None, None, p, 1568, p, 4, p, None, None, p, None) == abi.LG_ERR_INVALID
    assert "lg_estimator_step" in last_error(lib)
    assert lib.lg_mlp_set_output_activation(None, 1) == abi.LG_ERR_INVALID
    # abi.MLP_MAX_WIDTH, which parse_estimator_state holds the combination layer to, is the library's own limit: one more is refused for its width
    w, b = np.zeros((4, abi.MLP_MAX_WIDTH + 1), np.float32), np.zeros(4, np.float32)
    one = lambda a: (fp * 1)(a.ctypes.data_as(fp))          # noqa: E731
    assert not lib.lg_mlp_create(1, (C.c_int32 * 2)(abi.MLP_MAX_WIDTH + 1, 4), one(w), one(b), 0, 0)
    assert "layer width out of range (1..%d)" % abi.MLP_MAX_WIDTH in last_error(lib)
    mlp = lib.lg_mlp_create(1, (C.c_int32 * 2)(abi.MLP_MAX_WIDTH, 4), one(w[:, :-1].copy()), one(b), 0, 0)
    assert mlp or "layer width" not in last_error(lib)          # without a device it fails later, for that reason
    if mlp:
        lib.lg_mlp_destroy(mlp)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_estimator_kernels_do_not_spill_and_fit_the_lds():
    """csrc/lg_estimator.hip.  LDS bar: 160 KB per compute unit; the conv kernel is meant to run several workgroups per compute unit (two waves per
    SIMD at least), so one workgroup may take at most half of it."""
    blocks = kernel_metadata("lg_estimator.hip")
    kernels = ("conv_gemm_kernel", "pool_flatten_kernel", "cat_columns_kernel")
    check_no_spill_no_scratch(blocks, kernels, 80 * 1024)
    for part in kernels:
        assert kernel(blocks, part)["vgpr_count"] <= 128, part          # 256 lanes x 128 registers: two workgroups' waves per SIMD

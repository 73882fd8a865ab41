"""What tests/test_wide_input_power.py (CPU) and tests/test_hip_wide_input.py (GPU) share: the networks whose input row is wider than one 512-column
slab (`lg_mlp_create_wide`, include/lgpolicy.h).  Weights, rows, the float64 reference and the bar max(2e-5, 4 x yardstick) are those of
tests/policy_sweep.py (`case`, which also asserts that the floor binds and that the outputs are O(1)).  No GPU, no test functions.

Input widths: one past a slab (513), 64-padding one short of / at a second block of the second slab (577, 578: the raycast task's row), one short of,
at and one past two slabs (1023, 1024, 1025), three full slabs (1536), one short of and at the bound of four (2047, 2048).  First layers of 16 columns (one chunk: seven waves idle), 1, 33, 64, 65 and 512 (four chunks per wave); L = 1, 2 and 4."""
SLAB = 512
DIMS = [[513, 16], [577, 1], [578, 512, 256, 128, 18], [1023, 33, 7], [1024, 64, 12], [1025, 17, 1], [1536, 65, 3], [2047, 16], [2048, 512, 32]]
OTHER_ACT_CASES = [([578, 512, 256, 128, 18], "tanh"), ([1023, 33, 7], "selu")]
FORWARD_CASES = [(d, "elu") for d in DIMS] + OTHER_ACT_CASES
ROWS = (1, 33, 70)
# (actor, critic): a wide and a narrow network in one launch, in both orders, and two wide ones
ACT_PAIRS = [([578, 64, 18], [578, 33, 1]), ([1025, 17, 6], [48, 64, 1]), ([235, 129, 12], [2048, 512, 1])]
ACT_CALLS = (1, (1 << 32) + 7)
# layer-0 columns around every slab and 64-block edge a listed width has
COLUMNS = (0, 63, 64, 511, 512, 513, 575, 576, 1023, 1024, 1535, 1536, -1)          # -1: K - 1


def columns_of(K):
    return sorted({K - 1 if c < 0 else c for c in COLUMNS if c < K})

"""The software x87 model on the device: every operation of csrc/x87.h against the machine's long double over the
operations corpus, and the product's k_levinson over thousands of caller-made tables at once -- every Q15 word, every
`used`, every slot it must skip -- against the oracle (tests/x87recipes.py; entry points: csrc/k_x87_hooks.hip, in
liblacx_hooks.so only)."""
import pytest

import x87dev
import x87recipes as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    pkg.lacx.use_library(pkg.lacx.HOOKS_LIB_PATH)
    d = None
    try:
        d = x87dev.Device(pkg.lacx)
        yield d
    finally:
        if d is not None:
            d.close()
        pkg.lacx.use_library(None)


def test_device_x87_equals_long_double_on_the_operations_corpus(dev):
    """The device compile of x87.h (its own mul64x64 and clz64, div96by64's estimate under the device's contraction rules)
    in a kernel of its own: about 2^20 operand pairs, seven operations each, no tolerance."""
    c, want = X.ops_corpus(), X.ops_expected()
    for call in range(2):
        X.compare_ops(c, want, dev.ops(c), f"device, call {call}")


@pytest.mark.parametrize("depth", (16, 24))
def test_k_levinson_equals_oracle_on_every_table(dev, depth):
    """k_levinson as launch_analysis launches it, one-stream sets and stream tables: the LpcSet array byte for byte --
    the oracle's five candidates where the kernel must write (pad 0, zeros above `used` and at index 0, candidates
    above a short block's highest valid order skipped), the sentinel everywhere else.  Every launch twice on the same
    handle."""
    for pl in X.placements(depth):
        want = X.expected_lpcs(depth, pl)
        for call in range(2):
            X.compare_lpcs(pl, want, dev.levinson(pl), f"{depth}-bit magnitudes, call {call}")

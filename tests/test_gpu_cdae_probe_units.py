"""The 32-lane instances of cdae_sampled_decode_kernel (H <= 256: EPL = 4 and 8, a masked tail at H = 100 and 132, both
exact widths) on the probe-unit inputs of tests/cdae_wide_cases.py, with gradients and loss only, against the float64
reference of tests/cdae_ref64.py at its bars.  They share their slot code with the 64-lane instances; on these inputs
a hidden unit lost from z . W_o[i] — a register slot, lane 0 or lane 31, the last valid unit — crosses a bar
(tests/test_cdae_wide_host.py shows it without a GPU)."""
import pytest

import cdae_wide_cases as W
from test_gpu_cdae_wide import _decoder_with_gradients, _loss_only

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,I,H,act,with_bo,long", W.NARROW_PROBE_DECODE_CASES)
def test_narrow_decoder_on_the_probe_units(device, B, I, H, act, with_bo, long):
    """cdae_sampled_decode_kernel<32, 4 | 8, false, false>: 7 splits on short rows at H = 100, 128, 132 and 256, 8 splits
    on the long rows at 128 and 256."""
    _decoder_with_gradients(device, W.probe_decode_case(B, I, H, act, with_bo, long), B, I, H, act, "narrow probe units")


@pytest.mark.parametrize("B,I,H,act", W.NARROW_PROBE_LOSS_ONLY_CASES)
def test_narrow_loss_only_decoder_on_the_probe_units(device, B, I, H, act):
    """cdae_sampled_decode_kernel<32, 4 | 8, false, true> on the long rows and the settle() rows, then the loss
    finalizers on its partials."""
    _loss_only(device, W.probe_decode_case(B, I, H, act, True, True, settle=True), B, I, H, act,
               "narrow probe units, loss only")

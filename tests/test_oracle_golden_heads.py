"""The CPU oracle against the reference at more than eight heads (tests/golden/make_golden_heads.py: 9, 12, 16 and 32 heads): the check of
test_oracle_golden.py on the four fixtures the sketch -> video gate is held to on the device at these head counts
(tests/test_gpu_head_heads.py).  Pins the yardstick; needs no GPU."""
import pytest

from tests.test_oracle_golden import test_head_forward_loss_backward

# (imported under its own name pytest would collect it here a second time with its own parameters)
_head = test_head_forward_loss_backward
del test_head_forward_loss_backward


@pytest.mark.parametrize('name', ['h9_video', 'h12_frame', 'h16_video', 'h32_frame'])
def test_head_forward_loss_backward_above_eight_heads(name):
    _head(name)

"""The CPU oracle against the reference at head widths above 32 (tests/golden/make_golden_dh64.py: two heads of 64 or of 48): the
checks of test_oracle_golden.py / test_oracle_encdec.py, on the four fixtures the wide attention kernels are held to on the device
(tests/test_gpu_head_dh64.py).  Pins the yardstick; needs no GPU."""
import pytest

from tests.test_oracle_encdec import (test_encdec_forward_backward,
                                      test_encdec_training_mode_dropout_matches_the_reference_under_its_own_masks)
from tests.test_oracle_golden import test_head_forward_loss_backward

# (imported under their own names pytest would collect them here a second time with their own parameters)
_head, _encdec, _encdec_train = (test_head_forward_loss_backward, test_encdec_forward_backward,
                                 test_encdec_training_mode_dropout_matches_the_reference_under_its_own_masks)
del test_head_forward_loss_backward, test_encdec_forward_backward
del test_encdec_training_mode_dropout_matches_the_reference_under_its_own_masks


@pytest.mark.parametrize('name', ['dh64_video', 'dh48_frame'])
def test_head_forward_loss_backward_at_wide_heads(name):
    _head(name)


def test_encdec_forward_backward_at_head_width_64():
    _encdec('encdec_dh64_append_post')


def test_encdec_training_mode_dropout_at_head_width_64():
    _encdec_train('encdec_train_dh64_qry_pre')

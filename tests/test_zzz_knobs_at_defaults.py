"""LAST in collection order (the name sorts after tests/test_zz_rccl.py): the GPU suite flips tuning knobs on live contexts and every
accepted value gives equal results, so a knob left behind fails nothing -- later tests just stop testing the product's path."""
import pytest

from ringsnark_amd import _lib
from tests.test_tuning import DEFAULTS

pytestmark = pytest.mark.gpu


def test_the_suite_leaves_every_tuning_knob_at_its_default():
    assert {k: _lib.get_tuning(k) for k in _lib.tuning_keys()} == DEFAULTS

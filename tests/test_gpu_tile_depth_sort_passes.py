"""The cases of test_tile_depth_sort_passes.py (9-bit digits, the two passes with the fix-up, its fallback) on the HIP build."""
import pytest
import torch

import test_tile_depth_sort_passes as cases
from photo_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    capi.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("bits", cases.SPANS)
def test_every_length_at_every_span(dev, bits):
    cases.case_lengths_at_span(None, dev, bits)


def test_all_keys_equal(dev):
    cases.case_all_equal(None, dev)


@pytest.mark.parametrize("bits", cases.RUN_BITS)
def test_runs_of_equal_prefix(dev, bits):
    cases.case_runs(None, dev, bits)


def test_special_bit_patterns(dev):
    cases.case_special_patterns(None, dev)


def test_mixed_lists_in_one_launch(dev):
    cases.case_mixed(None, dev)

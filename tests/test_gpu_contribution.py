"""Per-Gaussian contribution statistics and the pruning by them on the MI355X (CPU twin: test_contribution.py): the checks of contribution_cases.py through libgsr_hip.so.  The
forward pass has no atomics and no order that depends on the schedule: its bit-exact checks hold on the device; gradients and
train steps are compared with the tolerances of test_gpu_depth_alpha.py."""
import pytest
import torch

import contribution_cases as cc
from photo_slam_amd import capi

pytestmark = pytest.mark.gpu
KS = [0.2, 0.6]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", KS)
def test_reference_input_condition_on_gpu(oracle, k, weighted):
    _dev()
    cc.check_input_condition(oracle, k, weighted)


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", KS)
def test_against_reference_on_gpu(oracle, k, weighted, flags):
    print(cc.check_reference(None, _dev(), oracle, k, weighted, flags))


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("k", KS)
def test_invariants_on_gpu(k, flags):
    print(cc.check_invariants(None, _dev(), k, flags))


@pytest.mark.parametrize("k", KS)
def test_bit_identity_on_gpu(k):
    cc.check_bit_identity(None, _dev(), k)


@pytest.mark.parametrize("flags", [32, 64 | 8])
def test_accumulate_on_gpu(flags):
    cc.check_accumulate(None, _dev(), 0.6, flags)


@pytest.mark.parametrize("flags", [32, 64])
def test_backward_after_contribution_forward_on_gpu(flags):
    cc.check_backward_after(None, _dev(), 0.6, flags, exact=False)


def test_options_on_gpu():
    cc.check_options(None, _dev())


def test_argument_errors_on_gpu():
    cc.check_argument_errors(None, _dev())


def test_hosts_python_on_gpu():
    cc.check_host_python(_dev(), exact=False)


def test_hosts_cpp_on_gpu():
    from tests.test_cpp_host import load_host
    cc.check_host_cpp(load_host("hip"), None, _dev(), exact=False)


def test_hosts_agree_on_gpu():
    from tests.test_cpp_host import load_host
    cc.check_hosts_agree(load_host("hip"), None, _dev())

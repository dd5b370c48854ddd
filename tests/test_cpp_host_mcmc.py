"""3DGS-MCMC relocation, growth and position noise through the LibTorch C++ host (GaussianModel::relocateDead / addNew /
addPositionNoise, TrainStep::mcmc_ / mcmc_cap_max_ / mcmc_noise_lr_ / mcmc_min_opacity_), driven through torch.ops.photoslam_amd and
compared with the Python mirror as tests/test_cpp_host.py does.  Shared checks: mcmc_cases.py."""
import pytest
import torch

import mcmc_cases as mc
from tests.test_cpp_host import load_host


def test_cpp_mcmc_matches_python(emu_lib_path):
    mc.check_host_cpp(load_host("emu"), emu_lib_path, torch.device("cpu"))


@pytest.mark.gpu
def test_cpp_mcmc_matches_python_on_gpu():
    mc.check_host_cpp(load_host("hip"), None, torch.device("cuda:0"))

"""The opacity / scale / isotropy regularisers through the LibTorch C++ host (RasterBackwardExtensions::geom_reg,
GaussianRasterizationExtensions::opacity_reg_ ..., TrainStep::opacity_reg_ / scale_reg_ / isotropic_reg_ / lastRegLosses()), driven
through torch.ops.photoslam_amd and compared with the Python mirror as tests/test_cpp_host.py does.  Shared checks:
geom_reg_cases.py."""
import pytest
import torch

import geom_reg_cases as gr
from tests.test_cpp_host import load_host


def test_cpp_train_step_with_regularisers_matches_python(emu_lib_path):
    gr.check_host_cpp(load_host("emu"), emu_lib_path, torch.device("cpu"))


@pytest.mark.gpu
def test_cpp_train_step_with_regularisers_matches_python_on_gpu():
    gr.check_host_cpp(load_host("hip"), None, torch.device("cuda:0"))

"""Camera pose gradients and pose refinement through the LibTorch C++ host (RasterBackwardExtensions::pose_grad,
GaussianRasterizerFunctionPose, PoseDelta, TrainStep::refinePose), driven through torch.ops.photoslam_amd and compared with the
Python mirror as tests/test_cpp_host.py does.  Shared checks: pose_grad_cases.py.

Refinement (pose_grad_cases.REFINE_SCENE at SH degree 1, 60 Adam steps, lr 2e-3, plain L1; % of the mean depth / degrees): start
1.75 % / 1.12 deg, bound 0.175 % / 0.112 deg; float64 reference loop 0.021 % / 0.014 deg (with the depth term at weight 0.01:
0.016 % / 0.016 deg).  Measured on the MI355X: C++ host 0.021 % / 0.023 deg, Python host on the same model 0.021 % / 0.019 deg; with
depth C++ 0.017 % / 0.018 deg, Python 0.016 % / 0.017 deg."""
import pytest
import torch

import pose_grad_cases as pg
from tests.test_cpp_host import load_host


def test_cpp_pose_gradient_matches_python(emu_lib_path):
    pg.check_pose_gradient_cpp(load_host("emu"), emu_lib_path, torch.device("cpu"))


@pytest.mark.parametrize("with_depth", [False, True])
def test_cpp_refine_pose_converges(emu_lib_path, oracle, with_depth):
    pg.check_refine_cpp(load_host("emu"), emu_lib_path, torch.device("cpu"), oracle, with_depth=with_depth)


@pytest.mark.gpu
def test_cpp_pose_gradient_and_refine_pose_on_gpu(oracle):
    ops = load_host("hip")
    dev = torch.device("cuda:0")
    pg.check_pose_gradient_cpp(ops, None, dev, exact=False)
    pg.check_refine_cpp(ops, None, dev, oracle)
    pg.check_refine_cpp(ops, None, dev, oracle, with_depth=True)

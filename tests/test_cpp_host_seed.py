"""Seeding Gaussians from an RGB-D frame through the LibTorch C++ host (GaussianModel::seedFromDepth, TrainStep::seedFromDepth and its
seed_* options), driven through torch.ops.photoslam_amd and compared with the Python mirror bit for bit.  Shared checks: seed_cases.py.

The C++ host is the one that leaves lazily stepped SH rows behind across an in-place append, so the train step after seeding is
checked here against a second C++ trainer that was handed the same rows through appendRows: identical bits on the emulator build; on
the MI355X the largest difference of a parameter or moment measured 1.5e-8 (the backward blend adds with float atomics there; bars rtol
1e-4, atol 1e-6 as tests/test_cpp_host.py)."""
import pytest
import torch

import seed_cases as sc
from tests.test_cpp_host import load_host


def test_cpp_seed_matches_python(emu_lib_path):
    sc.check_host_cpp(load_host("emu"), emu_lib_path, torch.device("cpu"))


@pytest.mark.gpu
def test_cpp_seed_matches_python_on_gpu():
    sc.check_host_cpp(load_host("hip"), None, torch.device("cuda:0"))

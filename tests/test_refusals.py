"""Every single-process-only feature of TrainStep is refused with a process group, on the C++ host and on the Python twin, with the
text the two share, and a refusal leaves nothing behind (refusal_cases.py); on the emulator build -- the code under test is host
code, the same in both builds."""
import pytest
import torch

import refusal_cases as rc
from photo_slam_amd import rasterize_points as rp

CPU = torch.device("cpu")


@pytest.fixture()
def emu(emu_lib_path, monkeypatch):
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    return emu_lib_path


def _host():
    from test_cpp_host import load_host
    return load_host("emu")


@pytest.fixture()
def one_rank_group(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        yield dist.group.WORLD.group_name
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", list(rc.FACTORED))
def test_refused_with_the_factored_exchange_cpp(emu, case):
    rc.check_refusal_cpp(_host(), CPU, case)


@pytest.mark.parametrize("case", list(rc.GROUP))
def test_refused_with_a_process_group_cpp(emu, one_rank_group, case):
    rc.check_refusal_cpp(_host(), CPU, case, group_name=one_rank_group)


@pytest.mark.parametrize("case", list(rc.FACTORED) + list(rc.GROUP))
def test_refused_with_a_process_group_python(emu, case):
    rc.check_refusal_python(emu, CPU, case)


def test_a_throwing_render_leaves_no_lazy_step_cpp(emu):
    rc.check_throwing_render_leaves_no_lazy_step(_host(), CPU)

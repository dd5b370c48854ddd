"""Forward-only rendering (GSR_FORWARD_ONLY) on the MI355X: the same image and radii as the training forward at the benchmark's
scales, the scratch sizes, the backward guard and the read-only lazy rows at C3 scale, and the viewer render between train steps
of both hosts.  (CPU twin: test_forward_only.py.)"""
import numpy as np
import pytest
import torch

import forward_only_cases as fo
from photo_slam_amd import capi
from photo_slam_amd import scene

pytestmark = pytest.mark.gpu
BG = np.array([0.2, 0.5, 0.1], np.float32)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("flags", [32, 64, 32 | 8])
@pytest.mark.parametrize("config,P", [("C1", None), ("C3", None), ("C4", None), ("C5", None)])
def test_forward_only_equals_training_forward_on_gpu(config, P, flags):
    dev = _dev()
    cl = scene.make_config(config, seed=1, P=P)
    fo.check_parity(None, dev, cl, cl.cameras[0], BG, flags)


def test_forward_only_scratch_guard_and_lazy_rows_at_c3_scale():
    dev = _dev()
    fo.check_sizes(capi.load())
    cl = scene.make_config("C3", seed=2)
    cam = cl.cameras[0]
    lib = capi.load()
    a = fo.inputs(cl, cam, BG, dev)
    R0, _, _, ws0, _ = fo.render(None, a, 0)
    R1, _, _, ws1, _ = fo.render(None, a, fo.FORWARD_ONLY)
    assert R0 == R1 and R0 >= 1 << 20
    assert ws1.requested[1] == lib.gsr_binning_bytes_for(R0, fo.FORWARD_ONLY) <= 0.35 * ws0.requested[1]
    fo.check_backward_guard(None, dev, cl, cam, BG)
    del a, ws0, ws1
    cl, cams = fo.lazy_scene(2_000_000, 1920, 1080, seed=3)
    fo.check_lazy_read_only(None, dev, cl, cams, BG, window=4)


def test_render_view_between_train_steps_on_gpu():
    """20 train steps with lazy SH Adam and a densification, with and without a render_view from another pose between every two
    steps.  The byte-exact part is checked around each view (run_*_interleaved): the model, its moments and its lazy state are
    byte-unchanged by the view, and the lazy state is alive after it exactly when it was before.  The two trajectories can only
    be compared loosely on the device: two runs of the SAME program differ in the last bits of a gradient there (the order of
    the quad-waves' LDS adds in the backward blend, tests/test_lazy_sh_adam.py), Adam turns a gradient whose sign is rounding
    noise into a whole step, and over 20 steps with a densification 0.5-1.5 % of the opacities were measured such steps apart
    between two runs.  (On the emulator the two trajectories are equal bit for bit: test_forward_only.py.)"""
    dev = _dev()
    cl, cams = fo.lazy_scene(20000, 320, 240, seed=21)
    from tests.test_cpp_host import load_host
    ops = load_host("hip")
    for run in (lambda v: fo.run_python_interleaved(None, dev, cl, cams, v), lambda v: fo.run_cpp_interleaved(ops, dev, cl, cams, v)):
        a, b = run(True), run(False)
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape, k
            if not torch.equal(x, y):
                off = (x - y).abs() > 1e-5 * float(y.abs().max()) + 1e-4 * y.abs()
                assert float(off.float().mean()) < 5e-2, (k, float(off.float().mean()))
                # (parameters: a few learning rates per step apart at most -- the largest is the opacity's 0.05)
                bound = 2 * 0.05 * 20 if k < 5 else 1e-2 * float(y.abs().max()) + 1e-6
                assert float((x - y).abs().max()) <= bound, (k, float((x - y).abs().max()))


def test_render_view_keeps_the_training_workspace_on_gpu():
    dev = _dev()
    cl, cams = fo.lazy_scene(20000, 320, 240, seed=22)
    fo.check_workspace(None, dev, cl, cams, exact=False)


def test_host_layers_switch_to_forward_only_on_gpu():
    dev = _dev()
    from tests.test_cpp_host import load_host
    cl = scene.make_config("C1", seed=4)
    fo.check_host_modes(load_host("hip"), None, dev, cl, cl.cameras[0], BG)

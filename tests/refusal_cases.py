"""The features of TrainStep that exist for a single process only, as one table: what switches each on, the call that must refuse
it, and the exact text of the refusal on the C++ host and on the Python twin.  A refusal leaves nothing behind (C++ host: step
counters, lazy-row counters, leaves and moments unchanged; the next ordinary step is the one a trainer that never saw the refused
call takes).  And the one exception path of renderAndBackward that has state to restore: a render that throws inside a lazy step."""
import pytest
import torch

import pose_grad_cases as pg
from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene

TAIL = " not supported with a process group"
# name: (options of trainer_set_options, attributes of the Python TrainStep, the call, the text; None = the same as the C++ host's)
# -- with the view-factored exchange on (C++) / world_size_ 2 (Python), which stand for a process group: nobody needs a second rank to ask
FACTORED = {
    "mcmc": ({"mcmc": 1.0}, {"mcmc_": True}, "step", "TrainStep: mcmc_ is" + TAIL, None),
    "absgrad": ({"absgrad": 1.0}, {"absgrad_": True}, "step", "TrainStep: absgrad_ is" + TAIL, None),
    "opacity_reg": ({"opacity_reg": 0.01}, {"opacity_reg_": 0.01}, "step", "TrainStep: the opacity / scale / isotropy regularisers are" + TAIL, None),
    "scale_reg": ({"scale_reg": 0.01}, {"scale_reg_": 0.01}, "step", "TrainStep: the opacity / scale / isotropy regularisers are" + TAIL, None),
    "isotropic_reg": ({"isotropic_reg": 0.01}, {"isotropic_reg_": 0.01}, "step", "TrainStep: the opacity / scale / isotropy regularisers are" + TAIL, None),
    "filter3d": ({"filter3d": 1.0}, {"filter3d_": True}, "step", "TrainStep: filter3d_ is" + TAIL, None),
    "seedFromDepth": ({}, {}, "seed", "TrainStep: seedFromDepth is" + TAIL, None),
}
# -- under a process group itself (C++: a one-rank gloo group)
GROUP = {
    "depth_loss": ({"depth_loss_weight": 0.5}, {"depth_loss_weight_": 0.5}, "depth_step",
                   "TrainStep: the depth loss is" + TAIL + " (depth_loss_weight_ must be 0)", None),
    "exposure": ({"optimize_exposure": 1.0}, {"optimize_exposure_": True}, "step", "TrainStep: exposure compensation is" + TAIL, None),
    "pruneUncontributing": ({}, {}, "prune", "TrainStep: pruneUncontributing is" + TAIL, "TrainStep: prune_uncontributing is" + TAIL),
}
WARM_STEPS = 2   # before the refused call: the lazy SH rows then have counters a refusal could disturb


def refusal_scene():
    return scene.make_cloud(300, 48, 32, 40.0, 40.0, seed=3, scale_k=0.35, n_views=2)


class Frames:
    """what the calls take: per camera the ops' arguments, a target image and a depth target; one full mask"""

    def __init__(self, cl, dev):
        self.args = [pg._cam_args(c, dev) for c in cl.cameras]
        H, W = cl.cameras[0].H, cl.cameras[0].W
        gen = torch.Generator().manual_seed(11)
        self.gts = [torch.rand(3, H, W, generator=gen).to(dev) for _ in cl.cameras]
        self.depths = [(torch.rand(H, W, generator=gen) * 6.0 + 1.0).to(dev) for _ in cl.cameras]
        self.mask = torch.ones(3, H, W, device=dev)
        self.batch = tuple(torch.stack([a[i] for a in self.args]) for i in range(3)) + tuple(self.args[0][3:])


def _step(ops, h, fr, k):
    ops.trainer_render_and_backward(h, *fr.args[k], fr.gts[k], fr.mask)
    ops.trainer_finish(h)


def _call(ops, h, fr, call):
    if call == "step":
        ops.trainer_render_and_backward(h, *fr.args[0], fr.gts[0], fr.mask)
    elif call == "depth_step":
        ops.trainer_render_and_backward_depth(h, *fr.args[0], fr.gts[0], fr.mask, fr.depths[0])
    elif call == "seed":
        ops.trainer_seed_from_depth(h, *fr.args[0], fr.gts[0], fr.depths[0], 5)
    else:
        ops.trainer_prune_uncontributing(h, *fr.batch, 0.1, 1)


def _untouched(ops, h):
    """step counters, lazy-row counters, and the leaves, moments and row counters as they are (trainer_state: nothing is brought
    up to date; its uint8 tail is the workspace, whose padding is the allocator's)"""
    return [torch.tensor(ops.trainer_steps(h)), ops.trainer_features_row_step(h)] + \
        [t.clone() for t in ops.trainer_state(h) if t.dtype != torch.uint8]


_after_one_more = {}


def params_of_an_unrefused_trainer(ops, cl, fr, dev):
    """WARM_STEPS + 1 ordinary steps of a trainer that never saw a refused call (computed once)"""
    if dev not in _after_one_more:
        h = pg.cpp_trainer(ops, cl, dev, deg=3)
        try:
            for i in range(WARM_STEPS + 1):
                _step(ops, h, fr, i % 2)
            _after_one_more[dev] = [p.detach().clone() for p in ops.trainer_params(h)]
        finally:
            ops.trainer_destroy(h)
    return _after_one_more[dev]


def check_refusal_cpp(ops, dev, case, group_name=None):
    """the refusal's exact text; nothing changed by it; with the feature and the exchange off again, the step of an unrefused trainer"""
    options, _, call, text, _ = (GROUP if group_name else FACTORED)[case]
    cl = refusal_scene()
    fr = Frames(cl, dev)
    want = params_of_an_unrefused_trainer(ops, cl, fr, dev)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        for i in range(WARM_STEPS):
            _step(ops, h, fr, i % 2)
        assert ops.trainer_features_row_step(h).numel() == cl.xyz.shape[0], "the warm steps were meant to leave lazy rows"
        if options:
            ops.trainer_set_options(h, options)
        if group_name:
            ops.trainer_set_process_group(h, group_name, True)
        else:
            ops.trainer_set_factored_exchange(h, True)
        before = _untouched(ops, h)
        with pytest.raises(RuntimeError) as e:
            _call(ops, h, fr, call)
        assert str(e.value) == text
        after = _untouched(ops, h)
        assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "a refusal changed the trainer"
        if group_name:
            ops.trainer_set_process_group(h, "", True)
            ops.trainer_set_options(h, {"fused_sh_adam": 1.0})   # (setProcessGroup switches it off, not the refusal)
        else:
            ops.trainer_set_factored_exchange(h, False)
        if options:
            ops.trainer_set_options(h, {k: 0.0 for k in options})
        _step(ops, h, fr, WARM_STEPS % 2)
        got = ops.trainer_params(h)
        assert len(got) == len(want) and all(torch.equal(a.detach(), b) for a, b in zip(got, want)), "a refusal left something behind"
    finally:
        ops.trainer_destroy(h)


def check_refusal_python(lib_path, dev, case):
    """the Python twin refuses with the same text (its own method name for pruneUncontributing) before the iteration advances"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    _, attrs, call, text, text_python = {**FACTORED, **GROUP}[case]
    cl = refusal_scene()
    fr = Frames(cl, dev)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = pg.python_trainer(cl, dev, deg=3)
        for k, v in attrs.items():
            assert hasattr(ts, k), k
            setattr(ts, k, v)
        ts.world_size_ = 2
        kf = GaussianKeyframe.from_camera(cl.cameras[0], dev)
        before = [p.detach().clone() for p in g.params_raw()]
        with pytest.raises(RuntimeError) as e:
            if call == "step":
                ts.trainForOneIteration(kf, fr.gts[0], fr.mask, sync_loss=False)
            elif call == "depth_step":
                ts.trainForOneIteration(kf, fr.gts[0], fr.mask, sync_loss=False, gt_depth=fr.depths[0])
            elif call == "seed":
                ts.seedFromDepth(kf, fr.gts[0], fr.depths[0], 5)
            else:
                ts.prune_uncontributing([kf], 0.1)
        assert str(e.value) == (text_python or text)
        assert ts.iteration_ == 0 and all(torch.equal(a, b.detach()) for a, b in zip(before, g.params_raw()))
    finally:
        rp._LIB_OVERRIDE = prev


def check_throwing_render_leaves_no_lazy_step(ops, dev):
    """A render that throws from inside a lazy step -- a float64 view matrix, which the rasterizer's wrapper refuses when it takes the
    float pointer, before any kernel -- must not leave the model in that step: the next training-path render brings the lazy rows up
    to date before it reads them, i.e. it shows exactly the model trainer_params() then returns, and so does trainer_render_view."""
    cl = refusal_scene()
    fr = Frames(cl, dev)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    h2 = None
    try:
        ops.trainer_set_options(h, {"lazy_sh_adam_window": 4.0})
        for k in (0, 1, 0):
            _step(ops, h, fr, k)
        behind = ops.trainer_features_row_step(h)
        assert behind.numel() and int(behind.min()) < int(behind.max()), "the steps were meant to leave rows behind"
        a = fr.args[1]
        with pytest.raises(RuntimeError):
            ops.trainer_render_and_backward(h, a[0].double(), *a[1:], fr.gts[1], fr.mask)
        image = ops.trainer_render(h, *a, False, False, True)[0].detach().clone()   # reads the SH rows through getFeatures()
        view = ops.trainer_render_view(h, *a).clone()
        p = [t.detach().clone() for t in ops.trainer_params(h)]
        h2 = ops.trainer_create(*p, 3, float(cl.extent), torch.zeros(3, device=dev))
        ops.trainer_set_options(h2, {"active_sh_degree": 3.0})
        assert torch.equal(image, ops.trainer_render(h2, *a, False, False, True)[0].detach()), "the model was left in a lazy step"
        assert torch.equal(view, ops.trainer_render_view(h2, *a))
    finally:
        ops.trainer_destroy(h)
        if h2 is not None:
            ops.trainer_destroy(h2)

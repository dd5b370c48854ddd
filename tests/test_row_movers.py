"""The row movers of the per-Gaussian kernels (csrc/shrows.h: wave_load_listed_rows, wave_adam_rows_rank1; csrc/preprocess_bwd.hip:
geom_adam_row) on the wave64 emulator, on the cases their loops can get wrong: halves of a wave's 64 rows with 0, 1, 3, 4, 5, 31
and 32 visible rows, a model that ends in the middle of a half and of a group of four rows, SH degrees 0-3, the lazy and the eager
mode of the fused SH step, and rows that are caught up by a forward pass after falling behind.

The reference is the oracle's gradients fed to torch.optim.Adam (oracle/cpu_trainer.py: the reference's step on the host), as in
tests/test_train_step.py::test_reference_cpu_train_step_equals_the_hip_train_step, and the tolerances are that test's:

  * parameters, in units of the learning rate: all but a fraction of 2e-3 of the elements within 1e-2 of a step (Adam normalises
    every gradient to a step of about lr, so a gradient whose sign is rounding noise flips a whole step);
  * both moments, with the tolerance that test uses for the gradient sums it compares with the reference (xyz_gradient_accum:
    rtol 1e-4, atol 1e-9): exp_avg is linear in the gradients like those sums; exp_avg_sq is compared through its square root,
    which is (atol 1e-9 would swallow a second moment of 1e-12 whole); and the same fraction of 2e-3 of the elements may miss
    it, for the same reason -- an element whose gradient is rounding noise.

A row mover that skips a row, steps it twice, reads the wrong row's moments or drops the last rows of a model misses these by the
whole value, on whole rows: 48 elements of a 300-Gaussian model are a fraction of 3e-3.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene
from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
from photo_slam_amd.trainer import TrainStep

W, H = 48, 32
# visible rows per half (32 consecutive rows) in the first keyframe; the model ends 13 rows into its last half: three groups of
# four rows and one row of a fourth
HALF_COUNTS = (0, 1, 3, 4, 5, 31, 32, 16, 7)
TAIL_ROWS, TAIL_VISIBLE = 13, 6
P_MODEL = 32 * len(HALF_COUNTS) + TAIL_ROWS
WINDOW = 4
NAMES = ("xyz", "features", "opacity", "scaling", "rotation")


def _visible(cl, cam, degree=3):
    from oracle import oracle
    res, _, radii = oracle.forward(np.zeros(3, np.float32), cl.xyz, cl.get_opacity(), cam.viewmatrix, cam.projmatrix, cam.campos,
                                   cam.tanfovx, cam.tanfovy, cam.H, cam.W, shs=cl.get_features(), sh_degree=degree,
                                   scales=cl.get_scaling(), rotations=cl.get_rotation())
    res.free()
    return radii > 0


@functools.lru_cache(maxsize=None)
def _designed_scene():
    """A cloud whose rows are drawn from a larger one so that the first keyframe sees exactly HALF_COUNTS rows of each half (a
    Gaussian's visibility depends on nothing but itself and the camera), and a second keyframe that looks elsewhere."""
    pool = scene.make_cloud(1500, W, H, 40.0, 40.0, seed=17, scale_k=0.35)
    cams = [pool.cameras[0],
            scene.make_camera(W, H, 40.0, 40.0, scene.look_rotation(0.3, 0.1), np.array([0.3, 0.0, -0.2]))]
    v0, v1 = _visible(pool, cams[0]), _visible(pool, cams[1])
    rng = np.random.default_rng(5)
    lit = list(rng.permutation(np.nonzero(v0)[0]))
    # the culled rows: those the SECOND keyframe sees first (they fall behind and are caught up by its forward pass)
    n_dark = P_MODEL - sum(HALF_COUNTS) - TAIL_VISIBLE
    late = list(rng.permutation(np.nonzero(~v0 & v1)[0])[:60])
    dark = late + list(rng.permutation(np.nonzero(~v0 & ~v1)[0])[:n_dark - len(late)])
    rng.shuffle(dark)
    rows = []
    for n_rows, n_lit in [(32, c) for c in HALF_COUNTS] + [(TAIL_ROWS, TAIL_VISIBLE)]:
        where = np.zeros(n_rows, bool)
        where[rng.permutation(n_rows)[:n_lit]] = True
        rows += [lit.pop() if w else dark.pop() for w in where]
    rows = np.array(rows)
    cl = scene.Cloud(pool.xyz[rows].copy(), pool.features_dc[rows].copy(), pool.features_rest[rows].copy(), pool.scaling[rows].copy(),
                     pool.rotation[rows].copy(), pool.opacity[rows].copy(), cams, extent=pool.extent)
    torch.manual_seed(3)
    gts = [torch.rand(3, H, W), torch.rand(3, H, W)]
    return cl, cams, gts


def test_the_designed_scene_has_the_halves_under_test():
    cl, cams, _ = _designed_scene()
    assert cl.xyz.shape[0] == P_MODEL and P_MODEL % 32 == TAIL_ROWS and TAIL_ROWS % 4 != 0
    v0, v1 = _visible(cl, cams[0]), _visible(cl, cams[1])
    per_half = [int(v0[a:a + 32].sum()) for a in range(0, P_MODEL, 32)]
    assert per_half == list(HALF_COUNTS) + [TAIL_VISIBLE]
    assert int((v1 & ~v0).sum()) >= 20      # rows the second keyframe lights after the first one culled them


@functools.lru_cache(maxsize=None)
def _reference(degree, steps, order):
    """The reference's step on the host cores with the oracle's gradients and torch.optim.Adam (oracle/cpu_trainer.py), at SH degree
    `degree`, over the keyframes `order`; parameters and both moments after `steps` steps."""
    from oracle import cpu_trainer
    cl, cams, gts = _designed_scene()
    torch.set_num_threads(2)
    cpu_trainer.oracle.build()
    l1_loss, ssim, _ = cpu_trainer._loss_ops()
    model = cpu_trainer.CpuModel(copy.deepcopy(cl), cl.extent)
    bg = np.zeros(3, np.float32)
    for it in range(1, steps + 1):
        k = order[it - 1]
        model.update_learning_rate(it)
        image, _, _, _ = cpu_trainer.render(model, cams[k], bg, sh_degree=degree)
        loss = 0.8 * l1_loss(image, gts[k]) + 0.2 * (1.0 - ssim(image, gts[k]))
        loss.backward()
        with torch.no_grad():
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
    m, v, _ = cpu_trainer._adam_state(model)
    d = lambda t: t.detach().clone()
    params = dict(xyz=d(model.xyz), features=torch.cat([d(model.features_dc), d(model.features_rest)], 1), opacity=d(model.opacity),
                  scaling=d(model.scaling), rotation=d(model.rotation))
    mom = lambda s: dict(xyz=d(s[0]), features=torch.cat([d(s[1]), d(s[2])], 1), opacity=d(s[3]), scaling=d(s[4]), rotation=d(s[5]))
    return params, mom(m), mom(v)


@functools.lru_cache(maxsize=None)
def _fused(lib, degree, window, steps, order):
    """TrainStep on the emulated kernels: fused SH step (lazy rows with `window` >= 2, every row at every step with 0) and fused
    geometry steps.  Returns parameters, moments, and lazy_row_step as it stood after every step (None in the eager mode)."""
    cl, cams, gts = _designed_scene()
    rp._LIB_OVERRIDE = lib
    try:
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device="cpu")
        opt = GaussianOptimizationParams()
        g.trainingSetup(opt)
        g.active_sh_degree_ = degree
        ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3), lazy_sh_adam_window=window)
        kfs = [GaussianKeyframe.from_camera(c, "cpu") for c in cams]
        mask = torch.ones(3, H, W)
        row_steps = []
        for it in range(1, steps + 1):
            k = order[it - 1]
            ts.trainForOneIteration(kfs[k], gts[k], mask)
            st = g.optimizer_.state[id(g._features)]
            row_steps.append(st["row_step"].clone() if "row_step" in st else None)
        params = dict(zip(NAMES, [p.detach().clone() for p in g.params()]))      # (reading features_ brings lazy rows up to date)
        m, v = {}, {}
        for n, p in zip(NAMES, g.params()):
            a, b = g.optimizer_.moments(p)
            m[n], v[n] = a.clone(), b.clone()
        assert g.optimizer_.state[id(g._features)]["step"] == steps
        return params, m, v, row_steps
    finally:
        rp._LIB_OVERRIDE = None


def _compare(got, want, what):
    cl = _designed_scene()[0]
    params, m, v = got[:3]
    rparams, rm, rv = want
    lrs = dict(xyz=0.00016 * cl.extent, features=0.0025, opacity=0.05, scaling=0.005, rotation=0.001)
    for n in NAMES:
        err = (params[n] - rparams[n]).abs() / lrs[n]
        frac = float((err > 1e-2).float().mean())
        print(f"{what} {n}: parameter error max {float(err.max()):.3g} lr, fraction beyond 1e-2 lr {frac:.3g}")
        assert frac < 2e-3, (what, n, float(err.max()), frac)
        for kind, a, b in (("exp_avg", m[n], rm[n]), ("sqrt(exp_avg_sq)", v[n].sqrt(), rv[n].sqrt())):
            off = (a - b).abs() > 1e-9 + 1e-4 * b.abs()
            frac = float(off.float().mean())
            print(f"{what} {n}: {kind} max |diff| {float((a - b).abs().max()):.3g} of max {float(b.abs().max()):.3g}, fraction beyond rtol 1e-4 {frac:.3g}")
            assert frac < 2e-3, (what, n, kind, frac)
        assert float(rm[n].abs().sum()) > 0     # the reference did step this tensor


@pytest.mark.parametrize("mode", ["lazy", "eager"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_row_movers_equal_adam_on_the_oracle_gradients(emu_lib_path, degree, mode):
    """One step and three steps (keyframes 0, 0, 1: the third forward pass catches up the rows the first keyframe culled)."""
    window = WINDOW if mode == "lazy" else 0
    order = (0, 0, 1)
    cl, cams, _ = _designed_scene()
    v0, v1 = _visible(cl, cams[0], degree), _visible(cl, cams[1], degree)
    for steps in (1, 3):
        got = _fused(emu_lib_path, degree, window, steps, order[:steps])
        _compare(got, _reference(degree, steps, order[:steps]), f"degree {degree} {mode} {steps} step(s)")
        row_steps = got[3]
        if mode == "eager":
            assert all(r is None for r in row_steps)
            continue
        # lazy_row_step: a row the step's keyframe sees has taken the step; no row is ahead, none further behind than the window
        for it, r in enumerate(row_steps, 1):
            seen = v0 if order[it - 1] == 0 else v1
            assert r.dtype == torch.int32 and r.shape == (P_MODEL,)
            assert int(r.max()) == it and int(r.min()) >= max(0, it - window)
            lit = torch.from_numpy(seen)
            # (the positions move by a fraction of a step of 7e-4: a Gaussian on the very edge of the view may change sides)
            assert float((r[lit] == it).float().mean()) > 0.98, (it, r[lit])
        if steps == 3:
            late = torch.from_numpy(v1 & ~v0)
            assert int((row_steps[1][late] < 2).sum()) >= 10, "no row is behind before the third step: the catch-up is not under test"
            assert float((row_steps[2][late] == 3).float().mean()) > 0.9


@pytest.mark.parametrize("degree", [1, 3])
def test_lazy_and_eager_row_movers_give_the_same_bits(emu_lib_path, degree):
    """The compact walk over the lit rows (lazy mode) and the masked walk over all rows (eager mode) are the same arithmetic."""
    a = _fused(emu_lib_path, degree, WINDOW, 3, (0, 0, 1))
    b = _fused(emu_lib_path, degree, 0, 3, (0, 0, 1))
    for k in range(3):
        for n in NAMES:
            assert torch.equal(a[k][n], b[k][n]), (k, n)

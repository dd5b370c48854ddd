"""Cost and effect of per-keyframe exposure compensation (gsr_l1_ssim_loss_exposure, TrainStep.optimize_exposure_).

Cost of the loss: ms per call of the plain entry, of the exposure entry and -- with --parent-lib, a libgsr_hip.so built from the
commit before the feature -- of the plain entry of that library, alternating in ONE process on the same buffers: the median of
--calls calls each behind --warmup, every call timed with HIP events.  The spread between the two plain entries is the yardstick
for the difference between plain and exposure.  At 1920 x 1080 and 752 x 480.
Cost of the step: the Python train step at C3 with optimize_exposure_ off and on (A B A B, median ms of --steps steps).
Effect: a C1-size scene trained for --train-iters iterations against targets whose exposure differs per keyframe (its own renders
behind a per-keyframe gain/offset), optimize_exposure_ off and on; the PSNR of the compensated renders -- render_view(kf,
apply_exposure=True) -- against the targets, mean over the keyframes.

  python tools/exposure_probe.py [--calls 200] [--warmup 20] [--steps 30] [--train-iters 300] [--parent-lib PATH]
                                 [--only loss|step|effect] [--sizes 1920x1080,752x480]

(The split of the three launches: rocprofv3 --kernel-trace --stats -- python tools/exposure_probe.py --only loss --sizes 1920x1080,
a run of its own.)
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from photo_slam_amd import capi, loss_utils, scene  # noqa: E402

SIZES = ((1920, 1080), (752, 480))


def loss_times(dev, W, H, calls, warmup, parent):
    lib = capi.load()
    g = torch.Generator().manual_seed(0)
    r, gt = (torch.rand(3, H, W, generator=g).to(dev) for _ in range(2))
    E = torch.tensor([[0.9, 0.08, -0.03, 0.02], [0.05, 1.1, 0.04, -0.03], [-0.02, 0.06, 0.85, 0.05]], device=dev)
    grad, ge, loss = torch.empty_like(r), torch.empty(12, device=dev), torch.empty(1, device=dev)
    scratch = torch.empty(int(lib.gsr_loss_exposure_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    plain = lambda L: L.gsr_l1_ssim_loss(r.data_ptr(), gt.data_ptr(), None, W, H, 0.2, grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), stream)
    forms = {"plain": lambda: plain(lib),
             "exposure": lambda: lib.gsr_l1_ssim_loss_exposure(r.data_ptr(), gt.data_ptr(), None, W, H, 0.2, E.data_ptr(), grad.data_ptr(),
                                                               ge.data_ptr(), loss.data_ptr(), scratch.data_ptr(), stream)}
    if parent is not None:
        forms["parent_plain"] = lambda: plain(parent)
    times = {k: [] for k in forms}
    order = list(forms)
    for k in range(warmup + calls):
        for name in order:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            assert forms[name]() == 0
            e.record()
            e.synchronize()
            if k >= warmup:
                times[name].append(s.elapsed_time(e))
        order = order[1:] + order[:1]   # (every form follows every other one equally often)
    out = {"W": W, "H": H, "calls": calls}
    for name, t in times.items():
        out[name] = {"median_ms": float(np.median(t)), "iqr_ms": float(np.percentile(t, 75) - np.percentile(t, 25))}
    return out


def make_trainer(cl, dev, optimize):
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    ts.optimize_exposure_ = optimize
    return g, ts


def step_ms(cl, dev, optimize, steps):
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    g, ts = make_trainer(cl, dev, optimize)
    cam = cl.cameras[0]
    kf = GaussianKeyframe.from_camera(cam, dev)
    torch.manual_seed(0)
    gt = torch.rand(3, cam.H, cam.W, device=dev)
    mask = torch.ones(3, cam.H, cam.W, device=dev)
    times = []
    for k in range(steps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
        e.record()
        torch.cuda.synchronize()
        if k >= 3:
            times.append(s.elapsed_time(e))
    return float(np.median(times)), float(np.percentile(times, 75) - np.percentile(times, 25))


def effect(dev, iters, n_views=4):
    """PSNR of the compensated renders after training against differently exposed targets, optimize_exposure_ off and on"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    truth = scene.make_config("C1", seed=1, n_views=n_views)
    _, ts0 = make_trainer(truth, dev, False)
    kfs0 = [GaussianKeyframe.from_camera(c, dev) for c in truth.cameras]
    gains = []
    targets = []
    for k, kf in enumerate(kfs0):
        gain = 0.7 + 0.6 * k / max(n_views - 1, 1)     # 0.7 ... 1.3, with a colour cast and an offset
        E = torch.tensor([[gain, 0, 0, 0.02 * (k - 1)], [0, gain * 0.95, 0, 0.0], [0, 0, gain * 1.05, -0.01 * k]], device=dev)
        gains.append(gain)
        targets.append(loss_utils.apply_exposure(ts0.render_view(kf).clone(), E).clone())
    out = {"config": "C1", "views": n_views, "iterations": iters, "gains": gains}
    start = copy.deepcopy(truth)                       # the true geometry with perturbed colours: the map has something to learn
    start.features_dc = start.features_dc + 0.1 * np.random.default_rng(3).standard_normal(start.features_dc.shape).astype(np.float32)
    for optimize in (False, True):
        _, ts = make_trainer(start, dev, optimize)
        kfs = [GaussianKeyframe.from_camera(c, dev) for c in truth.cameras]
        mask = torch.ones_like(targets[0])
        for it in range(iters):
            k = it % n_views
            ts.trainForOneIteration(kfs[k], targets[k], mask, sync_loss=False)
        psnr = [float(loss_utils.psnr(ts.render_view(kf, apply_exposure=True).clamp(0, 1), t.clamp(0, 1))) for kf, t in zip(kfs, targets)]
        out["optimize_on" if optimize else "optimize_off"] = {"psnr_mean": float(np.mean(psnr)), "psnr": psnr}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--train-iters", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES), help="W x H of the loss calls, comma separated")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.only in ("", "loss"):
        parent = None
        if args.parent_lib:   # (only the plain entry is called: the library predates the rest of capi's list)
            import ctypes as C
            parent = C.CDLL(os.path.abspath(args.parent_lib))
            parent.gsr_l1_ssim_loss.restype = C.c_int
            parent.gsr_l1_ssim_loss.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4
        for (W, H) in (tuple(int(v) for v in sz.split("x")) for sz in args.sizes.split(",")):
            print(json.dumps({"loss": loss_times(dev, W, H, args.calls, args.warmup, parent)}), flush=True)
    if args.only in ("", "step"):
        cl = scene.make_config("C3", seed=1)
        t = [step_ms(cl, dev, o, args.steps) for o in (False, True, False, True)]
        print(json.dumps({"train_step_ms": {"config": "C3", "optimize_off": [t[0][0], t[2][0]], "optimize_on": [t[1][0], t[3][0]],
                                            "iqr": [x[1] for x in t]}}), flush=True)
        del cl
        torch.cuda.empty_cache()
    if args.only in ("", "effect"):
        print(json.dumps({"effect": effect(dev, args.train_iters)}), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the monocular depth-prior loss (gsr_depth_prior_loss) and of the train step with it.

Cost of the loss: ms per call of the four space x mode combinations, of the fit-only call, of gsr_depth_l1_loss of the same build and
of the same two losses written in ATen on the device (forward + autograd backward), alternating in ONE process on the same buffers:
the median of --calls calls each behind --warmup, every call timed with HIP events.  At 1920 x 1080 and 752 x 480.  The algorithmic
traffic of the full call is 32 bytes per pixel (three maps read in each of two passes, two maps written).
Cost of the step: the Python train step at C3 without and with a prior (A B A B, median ms of --steps steps), aligned L1 and Pearson.

  python tools/depth_prior_probe.py [--calls 200] [--warmup 20] [--steps 30] [--only loss|step] [--sizes 1920x1080,752x480]
"""
import argparse
import copy
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from photo_slam_amd import capi, scene  # noqa: E402

SIZES = ((1920, 1080), (752, 480))
ALPHA_MIN = 0.5


def aten_prior(depth, alpha, q, weight, inverse, pearson):
    """the loss in ATen (float32, on the device), differentiable in depth and alpha"""
    ok = (alpha >= ALPHA_MIN) & (depth > 0) & torch.isfinite(q) & (q > 0)
    one = torch.ones((), dtype=depth.dtype, device=depth.device)
    d, a, qq = torch.where(ok, depth, one), torch.where(ok, alpha, one), torch.where(ok, q, one)
    r = a / d if inverse else d / a
    m = ok.to(depth.dtype)
    n = m.sum()
    qm, rm = (qq * m).sum() / n, (r * m).sum() / n
    dq, dr = (qq - qm) * m, (r - rm) * m
    sqq, sqr, srr = (dq * dq).sum(), (dq * dr).sum(), (dr * dr).sum()
    if pearson:
        return weight * (1.0 - sqr / torch.sqrt(sqq * srr))
    s = (sqr / sqq).detach()
    t = (rm - s * qm).detach()
    return weight * ((r - (s * qq + t)) * m).abs().sum() / depth.numel()


def loss_times(dev, W, H, calls, warmup):
    lib = capi.load()
    g = torch.Generator().manual_seed(0)
    alpha = (0.4 + 0.6 * torch.rand(H, W, generator=g)).to(dev)
    z = (1.0 + 3.0 * torch.rand(H, W, generator=g)).to(dev)
    depth = (z * alpha).contiguous()
    q = (0.5 / z + 0.1 + 0.02 * torch.rand(H, W, generator=g).to(dev)).contiguous()
    gd, ga, loss, fit = torch.empty_like(depth), torch.empty_like(depth), torch.empty(1, device=dev), torch.empty(4, device=dev)
    scratch = torch.empty(int(lib.gsr_depth_prior_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    scratch_l1 = torch.empty(int(lib.gsr_depth_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def prior(flags, grads=True):
        a = capi.DepthPriorArgs(W, H, depth.data_ptr(), alpha.data_ptr(), q.data_ptr(), None, flags, ALPHA_MIN, 0.1,
                                gd.data_ptr() if grads else None, ga.data_ptr() if grads else None, loss.data_ptr() if grads else None,
                                fit.data_ptr())
        return lambda: lib.gsr_depth_prior_loss(ctypes.byref(a), scratch.data_ptr(), stream)

    def aten(fn):
        d, a = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)

        def run():
            d.grad = a.grad = None
            fn(d, a).backward()
            return 0
        return run

    forms = {"l1": prior(0), "l1_inverse": prior(1), "pearson": prior(2), "pearson_inverse": prior(3), "fit_only": prior(1, False),
             "depth_l1_loss": lambda: lib.gsr_depth_l1_loss(depth.data_ptr(), z.data_ptr(), W, H, 0.1, 100.0, 0.1, gd.data_ptr(),
                                                            loss.data_ptr(), scratch_l1.data_ptr(), stream),
             "aten_l1_inverse": aten(lambda d, a: aten_prior(d, a, q, 0.1, True, False)),
             "aten_pearson_inverse": aten(lambda d, a: aten_prior(d, a, q, 0.1, True, True))}
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
    out = {"W": W, "H": H, "calls": calls, "algorithmic_bytes": 32 * W * H}
    for name, t in times.items():
        out[name] = {"median_ms": float(np.median(t)), "iqr_ms": float(np.percentile(t, 75) - np.percentile(t, 25))}
    return out


def step_ms(cl, dev, weight, pearson, steps):
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    ts.depth_prior_weight_, ts.depth_prior_pearson_ = weight, pearson
    cam = cl.cameras[0]
    kf = GaussianKeyframe.from_camera(cam, dev)
    torch.manual_seed(0)
    gt = torch.rand(3, cam.H, cam.W, device=dev)
    mask = torch.ones(3, cam.H, cam.W, device=dev)
    prior = 0.2 + torch.rand(cam.H, cam.W, device=dev)
    times = []
    for k in range(steps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ts.trainForOneIteration(kf, gt, mask, sync_loss=False, prior_depth=prior if weight else None)
        e.record()
        torch.cuda.synchronize()
        if k >= 3:
            times.append(s.elapsed_time(e))
    return float(np.median(times)), float(np.percentile(times, 75) - np.percentile(times, 25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", default="")
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES), help="W x H of the loss calls, comma separated")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.only in ("", "loss"):
        for (W, H) in (tuple(int(v) for v in sz.split("x")) for sz in args.sizes.split(",")):
            print(json.dumps({"loss": loss_times(dev, W, H, args.calls, args.warmup)}), flush=True)
    if args.only in ("", "step"):
        cl = scene.make_config("C3", seed=1)
        forms = [(0.0, False), (0.1, False), (0.1, True)]
        t = [step_ms(cl, dev, w, p, args.steps) for (w, p) in forms + forms]
        print(json.dumps({"train_step_ms": {"config": "C3", "without": [t[0][0], t[3][0]], "aligned_l1": [t[1][0], t[4][0]],
                                            "pearson": [t[2][0], t[5][0]], "iqr": [x[1] for x in t]}}), flush=True)


if __name__ == "__main__":
    main()

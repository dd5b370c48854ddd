"""Cost of the depth and alpha maps (gsr_forward_args.out_depth / out_alpha, gsr_backward_args.dL_ddepth / dL_dalpha) at C3 and a
C5 view: blend_fwd, blend_bwd and preprocess_bwd by gsr_profile (median of --reps forward + backward pairs each way, alternating),
and the Python train step (TrainStep.trainForOneIteration) without gt_depth and with the depth loss (median ms of --steps steps).

  python tools/depth_alpha_probe.py [--reps 20] [--steps 30] [--configs C3,C5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from photo_slam_amd import capi, scene  # noqa: E402
from photo_slam_amd import rasterize_points as rp  # noqa: E402
import forward_only_cases as fo  # noqa: E402

STAGES = ("blend_fwd", "blend_bwd", "preprocess_bwd")


def stage_times(a, cam, dev, maps, rng):
    """one profiled forward + backward: {stage: ms}"""
    lib = capi.load()
    H, W = cam.H, cam.W
    d = torch.empty((H, W), device=dev) if maps else None
    al = torch.empty((H, W), device=dev) if maps else None
    dpix = torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).to(dev)
    dD = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32)).to(dev) if maps else None
    dA = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32)).to(dev) if maps else None
    capi.profile_enable(lib, True)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, out_depth=d, out_alpha=al)
    rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                      a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix, a["sh"], 3,
                                      a["campos"], g, R, b, i, dL_ddepth=dD, dL_dalpha=dA)
    torch.cuda.synchronize()
    prof = capi.profile_read(lib)
    capi.profile_enable(lib, False)
    return {s: prof[s] for s in STAGES}


def train_ms(cl, dev, weight, steps):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    cam = cl.cameras[0]
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    ts.depth_loss_weight_, ts.depth_min_, ts.depth_max_ = weight, 1e-10, 100.0
    kf = GaussianKeyframe.from_camera(cam, dev)
    torch.manual_seed(0)
    gt = torch.rand(3, cam.H, cam.W, device=dev)
    gt_depth = torch.rand(cam.H, cam.W, device=dev) * 5.0
    mask = torch.ones(3, cam.H, cam.W, device=dev)
    times = []
    for k in range(steps + 3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ts.trainForOneIteration(kf, gt, mask, sync_loss=False, gt_depth=gt_depth if weight else None)
        e.record()
        torch.cuda.synchronize()
        if k >= 3:
            times.append(s.elapsed_time(e))
    return float(np.median(times))


def probe(name, reps, steps, dev):
    cl = scene.make_config(name, seed=1)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    rng = np.random.default_rng(0)
    runs = {False: [], True: []}
    stage_times(a, cam, dev, True, rng)   # (warm-up of both forms)
    stage_times(a, cam, dev, False, rng)
    for _ in range(reps):
        for maps in (False, True):
            runs[maps].append(stage_times(a, cam, dev, maps, rng))
    out = {"config": name, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H}
    for maps, key in ((False, "colour_only"), (True, "depth_alpha")):
        out[key] = {s: float(np.median([r[s] for r in runs[maps]])) for s in STAGES}
    out["ratio"] = {s: out["depth_alpha"][s] / out["colour_only"][s] for s in STAGES}
    del a
    torch.cuda.empty_cache()
    if steps:
        t0, t1 = train_ms(cl, dev, 0.0, steps), train_ms(cl, dev, 0.1, steps)
        out["train_step_ms"] = {"colour_only": t0, "depth_loss": t1, "ratio": t1 / t0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--configs", default="C3,C5")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        r = probe(name, args.reps, args.steps, dev)
        print(json.dumps(r), flush=True)
        c, d = r["colour_only"], r["depth_alpha"]
        print(f"{name}: " + ", ".join(f"{s} {c[s]:.3f} -> {d[s]:.3f} ms ({100 * (r['ratio'][s] - 1):+.1f} %)" for s in STAGES) +
              (f", train step {r['train_step_ms']['colour_only']:.3f} -> {r['train_step_ms']['depth_loss']:.3f} ms" if "train_step_ms" in r else ""),
              flush=True)


if __name__ == "__main__":
    main()

"""Cost and effect of anti-aliased rendering (GSR_ANTIALIAS, include/gsr.h).

Cost: preprocess_fwd and preprocess_bwd by gsr_profile (median of --reps forward + backward pairs each way, alternating) and the
Python train step (TrainStep(antialiasing=...), median ms of --steps steps), with and without the bit, at C3 and at one pyramid
level of it (C3's cloud rendered at a quarter of the width and height).
Effect: the level-consistency figure -- the mean alpha map of a cloud of mostly sub-pixel Gaussians at W x H and at W/4 x H/4 with
the same camera; |difference of the two means| with the bit, without it, and their ratio.

  python tools/antialias_probe.py [--reps 20] [--steps 30] [--configs C3] [--level 4]
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

STAGES = ("preprocess_fwd", "preprocess_bwd")


def stage_times(a, cam, dev, aa, rng):
    """one profiled forward + backward: {stage: ms}"""
    lib = capi.load()
    dpix = torch.from_numpy(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)).to(dev)
    capi.profile_enable(lib, True)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, antialiasing=aa)
    rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                      a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix, a["sh"], 3,
                                      a["campos"], g, R, b, i, antialiasing=aa)
    torch.cuda.synchronize()
    prof = capi.profile_read(lib)
    capi.profile_enable(lib, False)
    return {s: prof[s] for s in STAGES}


def train_ms(cl, cam, dev, aa, steps):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7, antialiasing=aa)
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


def level_camera(cam, level):
    """the same pose at 1 / level of the width and height (a pyramid level: same field of view)"""
    return scene.Camera(cam.W // level, cam.H // level, cam.tanfovx, cam.tanfovy, cam.viewmatrix, cam.projmatrix, cam.campos)


def probe(name, cam, cl, label, reps, steps, dev):
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    rng = np.random.default_rng(0)
    runs = {False: [], True: []}
    stage_times(a, cam, dev, True, rng)   # (warm-up of both forms)
    stage_times(a, cam, dev, False, rng)
    for k in range(reps):
        for aa in ((False, True) if k % 2 == 0 else (True, False)):
            runs[aa].append(stage_times(a, cam, dev, aa, rng))
    out = {"config": name, "view": label, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H}
    for aa, key in ((False, "plain"), (True, "antialiased")):
        out[key] = {s: float(np.median([r[s] for r in runs[aa]])) for s in STAGES}
        out[key + "_iqr"] = {s: float(np.percentile([r[s] for r in runs[aa]], 75) - np.percentile([r[s] for r in runs[aa]], 25)) for s in STAGES}
    del a
    torch.cuda.empty_cache()
    if steps:
        # A B A B: the spread between the two runs of one form is the yardstick for the difference between the forms
        t = [train_ms(cl, cam, dev, aa, steps) for aa in (False, True, False, True)]
        out["train_step_ms"] = {"plain": [t[0][0], t[2][0]], "antialiased": [t[1][0], t[3][0]], "iqr": [x[1] for x in t]}
    return out


def level_consistency(dev, P=200_000, W=1920, H=1080, level=4, scale_k=0.02, seed=8):
    from photo_slam_amd import capi as c
    fine = scene.make_cloud(P, W, H, 960.0, 960.0, seed=seed, scale_k=scale_k)
    cam = fine.cameras[0]
    means = {}
    for label, cm in (("fine", cam), ("coarse", level_camera(cam, level))):
        a = fo.inputs(fine, cm, np.zeros(3, np.float32), dev)
        for aa in (False, True):
            al = torch.zeros((cm.H, cm.W), device=dev)
            rp.RasterizeGaussiansCUDA(**a, raw_params=c.FORWARD_ONLY, out_alpha=al, antialiasing=aa)
            means[label, aa] = float(al.double().mean())
    d_with = abs(means["fine", True] - means["coarse", True])
    d_without = abs(means["fine", False] - means["coarse", False])
    return {"level_consistency": {"P": P, "W": W, "H": H, "level": level, "scale_k": scale_k,
                                  "mean_alpha": {f"{k[0]}_{'aa' if k[1] else 'plain'}": v for k, v in means.items()},
                                  "abs_diff_antialiased": d_with, "abs_diff_plain": d_without, "ratio": d_without / max(d_with, 1e-30)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--level", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        cl = scene.make_config(name, seed=1)
        cam = cl.cameras[0]
        for label, cm in (("full", cam), (f"level 1/{args.level}", level_camera(cam, args.level))):
            r = probe(name, cm, cl, label, args.reps, args.steps, dev)
            print(json.dumps(r), flush=True)
            p, q = r["plain"], r["antialiased"]
            print(f"{name} {label} {cm.W}x{cm.H}: " + ", ".join(f"{s} {p[s]:.4f} -> {q[s]:.4f} ms" for s in STAGES) +
                  (f", train step {r['train_step_ms']['plain']} -> {r['train_step_ms']['antialiased']} ms" if "train_step_ms" in r else ""),
                  flush=True)
    print(json.dumps(level_consistency(dev, level=args.level)), flush=True)


if __name__ == "__main__":
    main()

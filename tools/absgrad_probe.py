"""Cost of the absolute screen-space gradients (gsr_backward_args.dL_dmean2D_abs) in the backward pass and in the train step.

One forward pass (training form, raw parameters), then gsr_backward over and over on its buffers, alternating the cases in ONE
process, each call's blend_bwd and preprocess_bwd stages (long_run_sums + preprocess_bwd_kernel + sh_bwd_rows_kernel) read through
gsr_profile:
  parent_off  --parent-lib, a libgsr_hip.so built from the commit before the feature: the field does not exist
  off         this tree, dL_dmean2D_abs = NULL: the kernels and arguments of the parent, so it must sit inside the parent's
              interquartile range -- the yardstick for the case below
  on          the [P,2] output requested: the ABS instantiations of blend_bwd, long_run_sums and preprocess_bwd
Median and interquartile range of --calls calls per case behind --warmup; every case follows every other one equally often.
Then the Python train step (TrainStep.trainForOneIteration, fused optimizers and statistics, no densification) of two trainers
on copies of the model, absgrad_ off and on, alternating step by step: median milliseconds per step of --steps steps each.

  python tools/absgrad_probe.py [--calls 200] [--warmup 20] [--config C3] [--parent-lib PATH] [--steps 60]

(Per kernel: rocprofv3 --kernel-trace --stats -- python tools/absgrad_probe.py --calls 50 --steps 0, in a run of its own; the ABS
instantiations carry `true` as their last template argument.)
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

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

RAW = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
STAGES = ("blend_bwd", "preprocess_bwd")


def quartiles(t):
    q1, med, q3 = (float(np.percentile(t, q)) for q in (25, 50, 75))
    return {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "iqr_ms": q3 - q1}


def backward_stages(args, lib, cl, dev):
    cam = cl.cameras[0]
    P = cl.xyz.shape[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    a.update(opacity=fo._t(cl.opacity, dev), scales=fo._t(cl.scaling, dev), rotations=fo._t(cl.rotation, dev))
    dpix = torch.from_numpy(np.random.default_rng(0).standard_normal((3, cam.H, cam.W)).astype(np.float32)).to(dev)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=RAW)
    grads = {n: torch.empty((P, k), device=dev) for n, k in (("dL_dmean2D", 3), ("dL_dopacity", 1), ("dL_dcolor", 3), ("dL_dmean3D", 3),
                                                            ("dL_dsh", 48), ("dL_dscale", 3), ("dL_drot", 4))}
    ab = torch.empty((P, 2), device=dev)
    ba = capi.BackwardArgs()
    ba.P, ba.D, ba.M, ba.R, ba.width, ba.height = P, 3, 16, R, cam.W, cam.H
    ba.scale_modifier, ba.tan_fovx, ba.tan_fovy, ba.raw_params = 1.0, cam.tanfovx, cam.tanfovy, RAW
    for n in ("background", "means3D", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
        setattr(ba, n, a[n].data_ptr())
    ba.shs, ba.radii, ba.dL_dpix = a["sh"].data_ptr(), radii.data_ptr(), dpix.data_ptr()
    ba.geom_buffer, ba.binning_buffer, ba.image_buffer = g.data_ptr(), b.data_ptr(), i.data_ptr()
    for n, t in grads.items():
        setattr(ba, n, t.data_ptr())
    cases = {"off": (lib, None), "on": (lib, ab.data_ptr())}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.gsr_backward.restype = C.c_int
        parent.gsr_backward.argtypes = [C.POINTER(capi.BackwardArgs), C.c_void_p]   # (it reads the struct up to its own last field)
        cases = dict(parent_off=(parent, None), **cases)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for L in {id(v[0]): v[0] for v in cases.values()}.values():
        assert L.gsr_profile_enable(1) == 0
    names = [lib.gsr_profile_stage_name(k).decode() for k in range(lib.gsr_profile_stage_count())]
    idx = [names.index(s) for s in STAGES]
    ms = (C.c_float * len(names))()
    times = {c: {s: [] for s in STAGES} for c in cases}
    order = list(cases)
    for k in range(args.warmup + args.calls):
        for name in order:
            L, ptr = cases[name]
            ba.dL_dmean2D_abs = ptr
            st = L.gsr_backward(C.byref(ba), stream)
            assert st == 0, (name, st)
            assert L.gsr_profile_read(ms, len(names)) == 0
            if k >= args.warmup:
                for s, j in zip(STAGES, idx):
                    times[name][s].append(float(ms[j]))
        order = order[1:] + order[:1]   # (every case follows every other one equally often)
    torch.cuda.synchronize()
    lib.gsr_profile_enable(0)
    out = {c: {s: quartiles(times[c][s]) for s in STAGES} for c in cases}
    if "parent_off" in out:
        out["off_inside_parent_iqr"] = {s: bool(out["parent_off"][s]["q1_ms"] <= out["off"][s]["median_ms"] <= out["parent_off"][s]["q3_ms"])
                                        for s in STAGES}
    # how far the two statistics are apart, over the Gaussians some pixel blends (the last `on` call's arrays)
    signed = grads["dL_dmean2D"][:, :2].norm(dim=1)
    live = (radii > 0) & (signed > 0)
    ratio = ab[live].norm(dim=1) / signed[live]
    out["blended"] = int(live.sum())
    out["ratio_abs_over_signed"] = {"median": float(ratio.median()), "min": float(ratio.min())}
    return out


def train_steps(args, cl, dev):
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    cam = cl.cameras[0]
    kf = GaussianKeyframe.from_camera(cam, dev)
    torch.manual_seed(0)
    gt = torch.rand(3, cam.H, cam.W, device=dev)
    mask = torch.ones(3, cam.H, cam.W, device=dev)
    trainers = {}
    for name in ("off", "on"):
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        opt = GaussianOptimizationParams()
        g.trainingSetup(opt)
        ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
        ts.absgrad_ = name == "on"
        trainers[name] = ts
    times = {n: [] for n in trainers}
    order = list(trainers)
    for k in range(10 + args.steps):
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[name].trainForOneIteration(kf, gt, mask, sync_loss=False)
            torch.cuda.synchronize()
            if k >= 10:
                times[name].append(1e3 * (time.perf_counter() - t0))
        order = order[::-1]
    return {n: quartiles(t) for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("absgrad_probe.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    lib = capi.load()
    cl = scene.make_config(args.config, seed=1)
    cam = cl.cameras[0]
    out = {"config": args.config, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H, "calls": args.calls}
    out["backward"] = backward_stages(args, lib, cl, dev)
    if args.steps > 0:
        out["train_step"] = train_steps(args, cl, dev)
    print(json.dumps(out), flush=True)
    for case, stages in out["backward"].items():
        if isinstance(stages, dict) and "blend_bwd" in stages and isinstance(stages["blend_bwd"], dict):
            print(f"{case:11s} " + "  ".join(f"{s} {v['median_ms'] * 1e3:8.1f} us (IQR {v['iqr_ms'] * 1e3:.1f})" for s, v in stages.items()), flush=True)
    for case, v in out.get("train_step", {}).items():
        print(f"train step {case:4s} {v['median_ms']:.3f} ms (IQR {v['iqr_ms']:.3f})", flush=True)


if __name__ == "__main__":
    main()

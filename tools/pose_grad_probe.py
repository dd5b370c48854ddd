"""Cost of the camera pose gradients (gsr_backward_args.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos) at C1, C3 and a C5 view:
same-process alternating A/B of forward + backward pairs without and with the pose outputs -- the preprocess_bwd stage (the two
per-Gaussian kernels plus, with the outputs, the final-sum kernel) and the whole backward by gsr_profile, median of --reps pairs
each way -- and the wall-clock time of TrainStep.refinePose per iteration (median of --iters iterations).

  python tools/pose_grad_probe.py [--reps 20] [--iters 20] [--configs C1,C3,C5] [--lib PATH --without-only]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/pose_grad_probe.py --iters 0` in a run of its own
(the POSE instantiations carry `true` as their last template argument; pose_final_sum_kernel is the extra launch), and
`--kernel-stats FILE.csv` of a later call prints the rows of the backward's per-Gaussian kernels from rocprofv3's kernel_stats
table.  --lib PATH --without-only: the same "without" passes through another build of libgsr_hip.so (the parent commit's), so that
the unchanged kernels can be compared build against build.
"""
import argparse
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

STAGES = ("blend_bwd", "preprocess_bwd")
WITHOUT_ONLY = False
KERNELS = ("preprocess_bwd_kernel", "sh_bwd_rows_kernel", "pose_final_sum_kernel", "long_run_sums_kernel", "blend_bwd")


def print_kernel_stats(path):
    """the rows of rocprofv3's kernel_stats csv that belong to the backward pass: name, calls, average and median-free totals"""
    import csv
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if any(k in name for k in KERNELS):
                print(f"{name[:110]:110s} calls {row.get('Calls')} avg {float(row.get('AverageNs', 0)) / 1e3:9.2f} us "
                      f"min {float(row.get('MinNs', 0)) / 1e3:9.2f} max {float(row.get('MaxNs', 0)) / 1e3:9.2f}")


def stage_times(a, cam, dev, pose, dpix, ws):
    """one profiled forward + backward: {stage: ms}"""
    lib = capi.load()
    capi.profile_enable(lib, True)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a)
    rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                      a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix, a["sh"], 3,
                                      a["campos"], g, R, b, i, pose_grad=pose, workspace=ws)
    torch.cuda.synchronize()
    prof = capi.profile_read(lib)
    capi.profile_enable(lib, False)
    return {s: prof[s] for s in STAGES}


def refine_ms(cl, dev, iters):
    """wall-clock milliseconds per refinePose iteration (the whole call divided by its iterations, after a warm-up call)"""
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    cam = cl.cameras[0]
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    kf = GaussianKeyframe.from_camera(cam, dev)
    gt = ts.render_view(kf).clone()
    mask = torch.ones_like(gt)
    ts.refinePose(kf, gt, mask, 3, 1e-4, 1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ts.refinePose(kf, gt, mask, iters, 1e-4, 1e-4)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def probe(name, reps, iters, dev):
    cl = scene.make_config(name, seed=1)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    dpix = torch.from_numpy(np.random.default_rng(0).standard_normal((3, cam.H, cam.W)).astype(np.float32)).to(dev)
    ws = rp.RasterWorkspace()
    runs = {False: [], True: []}
    if not WITHOUT_ONLY:
        stage_times(a, cam, dev, True, dpix, ws)   # (warm-up of both forms)
    stage_times(a, cam, dev, False, dpix, None)
    for _ in range(reps):
        for pose in ((False,) if WITHOUT_ONLY else (False, True)):
            runs[pose].append(stage_times(a, cam, dev, pose, dpix, ws if pose else None))
    if WITHOUT_ONLY:
        runs[True] = runs[False]
    out = {"config": name, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H}
    for pose, key in ((False, "without"), (True, "with_pose")):
        out[key] = {s: float(np.median([r[s] for r in runs[pose]])) for s in STAGES}
        out[key + "_spread"] = {s: float(np.percentile([r[s] for r in runs[pose]], 90) - np.percentile([r[s] for r in runs[pose]], 10)) for s in STAGES}
    out["ratio"] = {s: out["with_pose"][s] / out["without"][s] for s in STAGES}
    del a
    torch.cuda.empty_cache()
    if iters:
        out["refine_pose_ms_per_iteration"] = refine_ms(cl, dev, iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="C1,C3,C5")
    ap.add_argument("--lib", default=None, help="another build of libgsr_hip.so (with --without-only)")
    ap.add_argument("--without-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="print the backward kernels' rows of a rocprofv3 kernel_stats csv and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        print_kernel_stats(args.kernel_stats)
        return
    global WITHOUT_ONLY
    WITHOUT_ONLY = args.without_only
    if args.lib:
        if not args.without_only:
            ap.error("--lib needs --without-only (another build does not know the pose outputs)")
        capi.HIP_LIB_PATH = os.path.abspath(args.lib)
        args.iters = 0
        # (a build from before the pose outputs lacks their one symbol: the binding asks for it when it loads a library)
        import ctypes

        class OlderBuild(ctypes.CDLL):
            def __getattr__(self, name):
                if name == "gsr_pose_grad_scratch_bytes":
                    return ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_int)(lambda P: 0)
                return super().__getattr__(name)
        cdll, ctypes.CDLL = ctypes.CDLL, OlderBuild
        try:
            capi.load()
        finally:
            ctypes.CDLL = cdll
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        r = probe(name, args.reps, args.iters, dev)
        print(json.dumps(r), flush=True)
        c, d = r["without"], r["with_pose"]
        print(f"{name}: " + ", ".join(f"{s} {c[s]:.3f} -> {d[s]:.3f} ms ({100 * (r['ratio'][s] - 1):+.1f} %)" for s in STAGES) +
              (f", refinePose {r['refine_pose_ms_per_iteration']:.3f} ms / iteration" if "refine_pose_ms_per_iteration" in r else ""),
              flush=True)


if __name__ == "__main__":
    main()

"""Cost and effect of the per-Gaussian contribution statistics (GSR_CONTRIBUTION, include/gsr.h) at C3 and a C5 view; one JSON file.

  (a) the plain forward-only render of this library against another build of it (--parent-lib: the parent commit's libgsr_hip.so),
      alternating A B A B, medians and quartiles of --reps renders each, HIP events -- the plain kernels are the same instructions;
  (b) the render with the statistics against (a), the same way; and, in a run of its own under rocprofv3 --kernel-trace --stats
      (a fresh child process: --trace-child), the split per kernel;
  (c) the effect: the share of radii > 0 Gaussians no pixel blends, the model size before and after
      TrainStep.prune_uncontributing over the cloud's views, and the PSNR of the views' renders after pruning against before.

  python tools/contribution_probe.py [--reps 200] [--configs C3,C5] [--parent-lib PATH] [--views 4] [--out profiles/contribution_probe.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

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

PRUNE_THRESHOLD = 1.0 / 255.0 / 16.0   # tests/contribution_cases.py: PRUNE_THRESHOLD


def quartiles(x):
    q = np.quantile(np.asarray(x, np.float64), [0.25, 0.5, 0.75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "iqr_ms": float(q[2] - q[0]), "n": len(x)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def renderers(a, dev, parent_lib):
    """{name: callable} of one forward-only render each: this library plain, the parent's plain, this library with the statistics"""
    P = a["means3D"].shape[0]
    ws = {k: rp.RasterWorkspace() for k in ("plain", "parent", "contribution")}
    out = (torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))
    this_lib = rp._lib

    def plain():
        rp.RasterizeGaussiansCUDA(**a, raw_params=capi.FORWARD_ONLY, workspace=ws["plain"])

    def contribution():
        rp.RasterizeGaussiansCUDA(**a, raw_params=capi.FORWARD_ONLY, workspace=ws["contribution"], out_weight_sum=out[0],
                                  out_weight_max=out[1], out_n_touched=out[2])

    r = {"plain": plain, "contribution": contribution}
    if parent_lib:
        other = capi.load(parent_lib)

        def parent():
            rp._lib = lambda: other   # (a tool's A/B handle: the same host code on another build of the library)
            try:
                rp.RasterizeGaussiansCUDA(**a, raw_params=capi.FORWARD_ONLY, workspace=ws["parent"])
            finally:
                rp._lib = this_lib
        r["parent"] = parent
    return r, out


def cost(name, reps, dev, parent_lib):
    cl = scene.make_config(name, seed=1)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    r, out = renderers(a, dev, parent_lib)
    for fn in r.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in r}
    for _ in range(reps):
        for k in ("plain", "parent", "contribution"):   # A B (C) A B (C) ...
            if k in r:
                t[k].append(timed(r[k]))
    res = {"config": name, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H, "forward_only_render": {k: quartiles(v) for k, v in t.items()}}
    f = res["forward_only_render"]
    if "parent" in f:
        res["plain_vs_parent"] = {"difference_ms": f["plain"]["median_ms"] - f["parent"]["median_ms"], "parent_iqr_ms": f["parent"]["iqr_ms"],
                                  "within_parent_iqr": abs(f["plain"]["median_ms"] - f["parent"]["median_ms"]) <= f["parent"]["iqr_ms"]}
    res["contribution_vs_plain"] = {"difference_ms": f["contribution"]["median_ms"] - f["plain"]["median_ms"],
                                    "ratio": f["contribution"]["median_ms"] / f["plain"]["median_ms"]}
    radii = rp.RasterizeGaussiansCUDA(**a, raw_params=capi.FORWARD_ONLY)[2]
    vis = radii > 0
    res["view0"] = {"visible": int(vis.sum()), "visible_untouched": int((vis & (out[2] == 0)).sum()),
                    "visible_untouched_share": float((vis & (out[2] == 0)).sum()) / max(1, int(vis.sum())),
                    "num_rendered": int(rp.RasterizeGaussiansCUDA(**a, raw_params=capi.FORWARD_ONLY)[0])}
    return res


def kernel_split(name):
    """rocprofv3 --kernel-trace --stats around a fresh child that renders 20 plain and 20 contribution views: average ns per kernel"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kp", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        fs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not fs:
            return {"error": p.stdout[-400:]}
        rows = {}
        for row in csv.DictReader(open(fs[0])):
            n = row["Name"]
            if any(s in n for s in ("blend_fwd_kernel", "contribution_reduce", "fill", "Fill", "memset")):
                rows[n[:110]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
        return rows


def trace_child(name):
    dev = torch.device("cuda:0")
    cl = scene.make_config(name, seed=1)
    a = fo.inputs(cl, cl.cameras[0], np.zeros(3, np.float32), dev)
    r, _ = renderers(a, dev, None)
    for _ in range(20):
        r["plain"]()
        r["contribution"]()
    torch.cuda.synchronize()


def effect(name, views, dev):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    cl = scene.make_config(name, seed=1, n_views=views)
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    kfs = [GaussianKeyframe.from_camera(c, dev) for c in cl.cameras]
    before = [ts.render_view(kf).clone() for kf in kfs]
    ts.score_contribution(kfs[:1])   # (warm-up)
    ms = timed(lambda: ts.score_contribution(kfs))
    _, wmax, touched, seen = ts.score_contribution(kfs)
    P0 = int(g.xyz_.shape[0])
    res = {"views": views, "score_contribution_ms": ms, "seen": int((seen > 0).sum()), "seen_untouched": int(((seen > 0) & (touched == 0)).sum())}
    for label, thr in (("1/255", 1.0 / 255.0), ("1/255/16", PRUNE_THRESHOLD)):
        g2 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        g2.trainingSetup(opt)
        t2 = TrainStep(g2, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
        n = t2.prune_uncontributing(kfs, thr)
        psnr = []
        for kf, b in zip(kfs, before):
            mse = float(((t2.render_view(kf) - b) ** 2).mean())
            psnr.append(10.0 * np.log10(1.0 / max(mse, 1e-20)))
        res["prune_" + label] = {"threshold": thr, "model_before": P0, "removed": int(n), "model_after": int(g2.xyz_.shape[0]),
                                 "psnr_db_min": float(min(psnr)), "psnr_db_mean": float(np.mean(psnr))}
        del g2, t2
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contribution_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", default=None)
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    dev = torch.device("cuda:0")
    results = []
    for name in args.configs.split(","):
        r = cost(name, args.reps, dev, args.parent_lib)
        torch.cuda.empty_cache()
        r["effect"] = effect(name, args.views, dev)
        torch.cuda.empty_cache()
        if not args.no_trace:
            r["kernels_us"] = kernel_split(name)
        results.append(r)
        print(json.dumps(r), flush=True)
        with open(args.out, "w") as f:   # (rewritten after every config: a time limit leaves what was measured)
            json.dump({"tool": "tools/contribution_probe.py", "reps": args.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()

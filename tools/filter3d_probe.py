"""Cost of the 3-D smoothing filter (GSR_FILTER_3D, gsr_filter3d_compute; include/gsr.h) at C3 and a C5 view:

  stages   preprocess_fwd and preprocess_bwd by gsr_profile, bit off against bit on (median of --reps forward + backward pairs each
           way, alternating, on one box).  With --no-filter only the bit-off path runs and no keyword of this feature is used: the
           form that also runs in a checkout of an earlier commit (--root), for the bit-off path against that commit and for an A/A
           pair of that commit (the box's scatter).
  compute  gsr_filter3d_compute at --compute-points Gaussians (2 M) for K = 8 and K = 100 cameras (median of --reps), next to one
           densifyAndPrune of the same model -- the yardstick for "negligible at an interval of 100".

  python tools/filter3d_probe.py [--reps 20] [--configs C3,C5] [--no-filter] [--root CHECKOUT] [--skip-compute]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--configs", default="C3,C5")
ap.add_argument("--no-filter", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--skip-compute", action="store_true")
ap.add_argument("--compute-points", type=int, default=2_000_000)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from photo_slam_amd import capi, scene  # noqa: E402
from photo_slam_amd import rasterize_points as rp  # noqa: E402
import forward_only_cases as fo  # noqa: E402

STAGES = ("preprocess_fwd", "preprocess_bwd")


def stage_times(a, cam, dev, filt, rng):
    """one profiled forward + backward: {stage: ms}; filt None = the calls without any keyword of this feature"""
    lib = capi.load()
    dpix = torch.from_numpy(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)).to(dev)
    kw = {} if filt is None else dict(filter_3D=filt)
    capi.profile_enable(lib, True)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, **kw)
    rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                      a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix, a["sh"], 3,
                                      a["campos"], g, R, b, i, **kw)
    torch.cuda.synchronize()
    prof = capi.profile_read(lib)
    capi.profile_enable(lib, False)
    return {s: prof[s] for s in STAGES}


def camera_rows(cams):
    rows = np.zeros((len(cams), 20), np.float32)
    for k, c in enumerate(cams):
        rows[k, :16] = c.viewmatrix.reshape(-1)
        rows[k, 16:] = [c.W / (2.0 * c.tanfovx), c.H / (2.0 * c.tanfovy), c.W, c.H]
    return rows


def probe_stages(name, reps, dev, with_filter):
    cl = scene.make_config(name, seed=1, n_views=3)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    rng = np.random.default_rng(0)
    filt = None
    if with_filter:
        filt = rp.filter3D(a["means3D"], torch.from_numpy(camera_rows(cl.cameras)).to(dev))
    forms = (None, filt) if with_filter else (None,)
    runs = {k: [] for k in range(len(forms))}
    for f in forms:   # (warm-up of every form)
        stage_times(a, cam, dev, f, rng)
    for _ in range(reps):
        for k, f in enumerate(forms):
            runs[k].append(stage_times(a, cam, dev, f, rng))
    out = {"config": name, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H, "root": ROOT}
    out["bit_off"] = {s: float(np.median([r[s] for r in runs[0]])) for s in STAGES}
    if with_filter:
        out["bit_on"] = {s: float(np.median([r[s] for r in runs[1]])) for s in STAGES}
        out["ratio"] = {s: out["bit_on"][s] / out["bit_off"][s] for s in STAGES}
    return out


def timed(fn, reps):
    times = []
    for k in range(reps + 2):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if k >= 2:
            times.append(s.elapsed_time(e))
    return float(np.median(times))


def probe_compute(P, reps, dev):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    out = {"P": P}
    for K in (8, 100):
        cl = scene.make_cloud(P, 1920, 1080, 960.0, 960.0, seed=1, n_views=K)
        xyz = torch.from_numpy(cl.xyz).to(dev)
        rows = torch.from_numpy(camera_rows(cl.cameras)).to(dev)
        buf = torch.empty(P, device=dev)
        out[f"filter3d_K{K}_ms"] = timed(lambda: rp.filter3D(xyz, rows, 0.2, out=buf), reps)
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    g.trainingSetup(GaussianOptimizationParams())
    for _ in range(2):   # (the first call builds the arena of the rebuilds: the second is the steady state)
        n = g.xyz_.shape[0]
        g.denom_.fill_(1.0)
        g.xyz_gradient_accum_.copy_(torch.rand(n, 1, device=dev) * 2.2e-4)   # (a tenth of the rows above the default threshold of 2e-4)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = g.densifyAndPrune(2e-4, 0.005, float(cl.extent), 0)
        e.record()
        torch.cuda.synchronize()
    out["densify_and_prune_ms"] = float(s.elapsed_time(e))
    out["densify_and_prune"] = {k: int(v) for k, v in r.items()}
    return out


def main():
    dev = torch.device("cuda:0")
    for name in [c for c in ARGS.configs.split(",") if c]:
        r = probe_stages(name, ARGS.reps, dev, not ARGS.no_filter)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if not ARGS.skip_compute and not ARGS.no_filter:
        print(json.dumps(probe_compute(ARGS.compute_points, ARGS.reps, dev)), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the fixed-budget map maintenance (3DGS-MCMC: GaussianModel.relocateDead / addNew / addPositionNoise) at C3, Python host.

Two questions, one process:

  1. a densification event.  On the same model (C3's cloud with --dead of its rows made dead and densification statistics that
     select about --selected of them for cloning or splitting), host wall clock around the call and a device synchronise:
       relocate        relocateDead + addNew at the cap (addNew returns 0): the steady state of a fixed-budget map, in place
       relocate_grow   relocateDead + addNew of 5 %: a growth event (the arena has the room: an in-place append)
       densify_prune   densifyAndPrune: select, one host read of the counts, the gather of every tensor and moment
     Every repetition starts from a fresh copy of the model (the copy is not timed); the three cases alternate.
  2. the noise launch.  A train step (fused, lazy SH rows, the benchmark's stationary workload: lr_scale = 0, so the noise scale
     is 0 too and the positions stay put while the randn and the kernel run in full) with mcmc_ off and on, alternating blocks of
     --steps steps behind --warmup, host wall clock per block behind a device synchronise.

  python tools/mcmc_probe.py [--config C3] [--reps 7] [--steps 100] [--blocks 6] [--warmup 20]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

__graft_entry__.load_package()
from photo_slam_amd import scene  # noqa: E402
from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams  # noqa: E402
from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams, GaussianRenderer  # noqa: E402
from photo_slam_amd.trainer import TrainStep  # noqa: E402


def summary(t):
    q1, med, q3 = (float(np.percentile(t, q)) for q in (25, 50, 75))
    return {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "n": len(t)}


def fresh_model(cl, dev, dead_rows, accum):
    g = GaussianModel.from_cloud(cl, device=dev)
    g.trainingSetup(GaussianOptimizationParams())
    # the state a map has in training: moments exist, the live tensors are the arena's (25 % headroom: a growth event appends in place)
    g._append_rows({n: getattr(g, n).detach()[:0] for n in g._PARAM_NAMES}, 0)
    with torch.no_grad():
        g.opacity_[dead_rows] = -8.0
    g.xyz_gradient_accum_.copy_(accum)
    g.denom_.fill_(1.0)
    return g


def event_costs(cl, dev, args):
    P = cl.xyz.shape[0]
    rng = np.random.default_rng(0)
    dead_rows = torch.from_numpy(rng.choice(P, int(P * args.dead), replace=False)).to(dev)
    accum = torch.zeros((P, 1), device=dev)
    accum[torch.from_numpy(rng.choice(P, int(P * args.selected), replace=False)).to(dev)] = 1.0   # (far above densify_grad_threshold_)
    gen = torch.Generator(device=dev).manual_seed(1)
    opt = GaussianOptimizationParams()
    times = {"relocate": [], "relocate_grow": [], "densify_prune": []}
    info = {}
    order = list(times)
    for rep in range(args.reps + 1):   # (the first repetition warms every kernel and allocation up and is dropped)
        for name in order:
            g = fresh_model(cl, dev, dead_rows, accum)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "densify_prune":
                r = g.densifyAndPrune(opt.densify_grad_threshold_, 0.005, float(cl.extent), 0, generator=gen)
                info[name] = {k: int(v) for k, v in r.items()}
            else:
                counts = g.relocateDead(0.005, generator=gen)
                added = g.addNew(P if name == "relocate" else 2 * P, generator=gen)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if name != "densify_prune":
                info[name] = {"counts": counts.cpu().tolist()[:4], "added": int(added), "points": int(g.xyz_.shape[0])}
            if rep:
                times[name].append(dt)
            del g
        order = order[1:] + order[:1]
    return {k: dict(summary(v), **info[k]) for k, v in times.items()}


def step_costs(cl, dev, args):
    cam = cl.cameras[0]
    g = GaussianModel.from_cloud(cl, device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    kf = GaussianKeyframe.from_camera(cam, dev)
    bg = torch.zeros(3, device=dev)
    pipe = GaussianPipelineParams()
    with torch.no_grad():
        gt = GaussianRenderer.render(kf, cam.H, cam.W, g, pipe, bg)[0].clone()
    mask = torch.ones_like(gt)
    ts = TrainStep(g, opt, pipe, bg, cameras_extent=cl.extent)
    ts.mcmc_cap_max_ = g.xyz_.shape[0]
    g.optimizer_.lr_scale = 0.0
    times = {"off": [], "on": []}
    for _ in range(args.warmup):
        for on in (False, True):
            ts.mcmc_ = on
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
    for b in range(2 * args.blocks):
        ts.mcmc_ = bool(b & 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
        torch.cuda.synchronize()
        times["on" if ts.mcmc_ else "off"].append((time.perf_counter() - t0) * 1e3 / args.steps)
    return {"step_mcmc_off": summary(times["off"]), "step_mcmc_on": summary(times["on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dead", type=float, default=0.05)
    ap.add_argument("--selected", type=float, default=0.05)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_probe.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    cl = scene.make_config(args.config, seed=1)
    out = {"config": args.config, "P": int(cl.xyz.shape[0]), "dead_fraction": args.dead, "selected_fraction": args.selected}
    out.update(event_costs(cl, dev, args))
    out.update(step_costs(copy.deepcopy(cl), dev, args))
    print(json.dumps(out), flush=True)
    for k in ("relocate", "relocate_grow", "densify_prune", "step_mcmc_off", "step_mcmc_on"):
        print(f"{k:14s} {out[k]['median_ms']:9.3f} ms  (quartiles {out[k]['q1_ms']:.3f} .. {out[k]['q3_ms']:.3f}, n = {out[k]['n']})", flush=True)


if __name__ == "__main__":
    main()

"""Cost of seeding Gaussians from an RGB-D frame (gsr_seed_select + gsr_seed_emit, GaussianModel.seedFromDepth) against the route the
library offered before: a boolean mask made in torch, gsr_reproject_depth_pinhole, boolean indexing, increasePcd (whose scales come
from a kNN over the new points).

At 1920 x 1080 and 752 x 480, with about --fractions of the pixels selected (alpha = 0 there, 1 elsewhere; depth = gt * alpha, so
that the depth rule selects nothing and both routes pick exactly the same pixels), on a model of --model-rows Gaussians that has
optimizer state and lives in the arena.  Every repetition starts from a fresh copy of the model (not timed); the routes alternate;
host wall clock around the call and a device synchronise, medians and quartiles:

  select_emit    gsr_seed_select, the one host read of the counts, gsr_seed_emit into rows that already have the room
  seed_host      GaussianModel.seedFromDepth: the same plus the arena append (re-seating of the leaves, zeroing of the statistics)
  parent_route   the torch mask (valid range, alpha threshold, the depth rule with torch.median), gsr_reproject_depth_pinhole
                 over the image, boolean indexing of points and colours, increasePcd

  python tools/seed_probe.py [--reps 7] [--fractions 0.1,1.0] [--model-rows 100000] [--out FILE]
"""
import argparse
import ctypes as C
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
from photo_slam_amd import capi, scene  # noqa: E402
from photo_slam_amd import operate_points as op  # noqa: E402
from photo_slam_amd import rasterize_points as rp  # noqa: E402
from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams  # noqa: E402

MIN_DEPTH, MAX_DEPTH, ALPHA_THRESHOLD, MEDIAN_FACTOR = 0.1, 100.0, 0.5, 50.0


def summary(t):
    q1, med, q3 = (float(np.percentile(t, q)) for q in (25, 50, 75))
    return {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "n": len(t)}


def fresh_model(cl, dev):
    g = GaussianModel.from_cloud(cl, device=dev)
    g.trainingSetup(GaussianOptimizationParams())
    g._append_rows({n: getattr(g, n).detach()[:0] for n in g._PARAM_NAMES}, 0)   # moments exist, the live tensors are the arena's
    return g


def frame(W, H, fraction, dev):
    gen = torch.Generator(device=dev).manual_seed(W + H)
    gt = torch.rand((H, W), generator=gen, device=dev) * 4.0 + 0.5
    alpha = (torch.rand((H, W), generator=gen, device=dev) >= fraction).float()
    image = torch.rand((3, H, W), generator=gen, device=dev)
    return gt, alpha, (gt * alpha).contiguous(), image


def parent_route(g, gt, alpha, depth, image, intr, W):
    valid = (gt > MIN_DEPTH) & (gt < MAX_DEPTH)
    e = (gt - depth).abs()
    T = MEDIAN_FACTOR * e[valid].median()
    mask = (valid & ((alpha < ALPHA_THRESHOLD) | ((depth > gt) & (e > T)))).reshape(-1)
    pts = op.reprojectDepthPinhole(gt.reshape(-1), mask, intr, W)
    return g.increasePcd(pts[mask], image.reshape(3, -1).t()[mask], 1)


def seed_host(g, gt, alpha, depth, image, vm, intr):
    return g.seedFromDepth(gt, image, alpha, depth, vm, *intr, 1, 1 << 30, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                           alpha_threshold=ALPHA_THRESHOLD, depth_median_factor=MEDIAN_FACTOR)


def select_emit(lib, g, room, gt, alpha, depth, image, vm, intr, scratch, counts):
    """the two C-ABI calls and the read between them, into `room` (rows behind P of buffers that are large enough)"""
    H, W = gt.shape
    stream = rp._stream_ptr(gt)
    a = capi.SeedSelectArgs()
    a.width, a.height, a.alpha, a.depth, a.gt_depth = W, H, alpha.data_ptr(), depth.data_ptr(), gt.data_ptr()
    a.min_depth, a.max_depth, a.alpha_threshold, a.depth_error_median_factor, a.stride = MIN_DEPTH, MAX_DEPTH, ALPHA_THRESHOLD, MEDIAN_FACTOR, 1
    capi.check(lib, lib.gsr_seed_select(C.byref(a), scratch.data_ptr(), counts.data_ptr(), stream), "gsr_seed_select")
    n = counts.tolist()[0]
    e = capi.SeedEmitArgs()
    e.width, e.height, e.stride, e.n_selected, e.n_emit, e.P, e.features_row_floats = W, H, 1, n, n, 0, 48
    e.gt_depth, e.image, e.viewmatrix = gt.data_ptr(), image.data_ptr(), vm.data_ptr()
    e.fx, e.fy, e.cx, e.cy = intr
    e.scale_factor, e.init_opacity, e.iteration = 1.0, 0.5, 1
    for i, (p, m1, m2) in enumerate(room["params"]):
        e.param[i], e.exp_avg[i], e.exp_avg_sq[i] = p.data_ptr(), m1.data_ptr(), m2.data_ptr()
    e.exist_since_iter = room["exist"].data_ptr()
    for k in range(3):
        e.stats[k] = room["stats"][k].data_ptr()
    capi.check(lib, lib.gsr_seed_emit(C.byref(e), scratch.data_ptr(), stream), "gsr_seed_emit")
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fractions", default="0.1,1.0")
    ap.add_argument("--model-rows", type=int, default=100000)
    ap.add_argument("--sizes", default="1920x1080,752x480")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seed_probe.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    lib = rp._lib()
    out = {"model_rows": args.model_rows, "cases": []}
    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        cl = scene.make_cloud(args.model_rows, W, H, 0.5 * W, 0.5 * W, seed=1)
        cam = cl.cameras[0]
        vm = torch.from_numpy(cam.viewmatrix).to(dev).contiguous()
        intr = (W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy), (W - 1) / 2.0, (H - 1) / 2.0)
        scratch = torch.empty(int(lib.gsr_seed_scratch_bytes(W, H)) + 256, dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=torch.int32, device=dev)
        n_px = W * H
        mk = lambda *s: torch.empty((n_px,) + s, device=dev)
        room = dict(params=[tuple(mk(*s) for _ in range(3)) for s in ((3,), (16, 3), (1,), (3,), (4,))],
                    stats=[mk(1), mk(1), mk()], exist=torch.empty(n_px, dtype=torch.int32, device=dev))
        for fraction in (float(f) for f in args.fractions.split(",")):
            gt, alpha, depth, image = frame(W, H, fraction, dev)
            times = {"select_emit": [], "seed_host": [], "parent_route": []}
            rows = {}
            order = list(times)
            for rep in range(args.reps + 1):   # (the first repetition warms every kernel and allocation up and is dropped)
                for name in order:
                    g = fresh_model(cl, dev) if name != "select_emit" else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name == "select_emit":
                        n = select_emit(lib, g, room, gt, alpha, depth, image, vm, intr, scratch, counts)
                    elif name == "seed_host":
                        n = seed_host(g, gt, alpha, depth, image, vm, intr)
                    else:
                        n = parent_route(g, gt, alpha, depth, image, intr, W)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    rows[name] = int(n)
                    if rep:
                        times[name].append(dt)
                    del g
                order = order[1:] + order[:1]
            assert len(set(rows.values())) == 1, rows   # the routes insert the same number of Gaussians
            case = {"W": W, "H": H, "fraction": fraction, "rows": rows["seed_host"]}
            case.update({k: summary(v) for k, v in times.items()})
            out["cases"].append(case)
            print(f"{W}x{H} {rows['seed_host']:8d} rows: " + "  ".join(f"{k} {case[k]['median_ms']:.3f} ms" for k in times), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

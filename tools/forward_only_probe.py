"""Forward-only rendering (GSR_FORWARD_ONLY, include/gsr.h) against the training forward at C1, C3 and a C5 view: the scratch
bytes each requests, the median of 50 renders each way (events around each render, buffers allocated per call as the reference
does), blend_fwd by gsr_profile, and torch.cuda.max_memory_allocated for one render.

  python tools/forward_only_probe.py [--renders 50]
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


def probe(name, renders, dev):
    cl = scene.make_config(name, seed=1)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    lib = capi.load()
    out = {"config": name, "P": int(cl.xyz.shape[0]), "W": cam.W, "H": cam.H}
    for mode, flags in (("training", 0), ("forward_only", fo.FORWARD_ONLY)):
        R, _, _, ws, _ = fo.render(None, a, flags)
        del ws
        torch.cuda.synchronize()
        times = []
        for _ in range(renders + 3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rp.RasterizeGaussiansCUDA(**a, raw_params=flags)   # (per-call buffers, as the reference's resizeFunctional)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        capi.profile_enable(lib, True)
        rp.RasterizeGaussiansCUDA(**a, raw_params=flags)
        torch.cuda.synchronize()
        prof = capi.profile_read(lib)
        capi.profile_enable(lib, False)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        rp.RasterizeGaussiansCUDA(**a, raw_params=flags)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        out[mode] = {"R": R, "binning_bytes": int(lib.gsr_binning_bytes_for(R, flags)),
                     "image_bytes": int(lib.gsr_image_bytes_for(cam.W, cam.H, flags)),
                     "median_ms": float(np.median(times[3:])), "blend_fwd_ms": prof["blend_fwd"],
                     "max_memory_allocated_MB": peak / 2**20}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--renders", type=int, default=50)
    ap.add_argument("--configs", default="C1,C3,C5")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        r = probe(name, args.renders, dev)
        print(json.dumps(r))
        t, f = r["training"], r["forward_only"]
        print(f"{name}: binning {t['binning_bytes'] / 2**20:.1f} -> {f['binning_bytes'] / 2**20:.1f} MiB, image "
              f"{t['image_bytes'] / 2**20:.2f} -> {f['image_bytes'] / 2**20:.2f} MiB, render {t['median_ms']:.3f} -> "
              f"{f['median_ms']:.3f} ms, blend_fwd {t['blend_fwd_ms']:.3f} -> {f['blend_fwd_ms']:.3f} ms, peak "
              f"{t['max_memory_allocated_MB']:.0f} -> {f['max_memory_allocated_MB']:.0f} MiB", flush=True)


if __name__ == "__main__":
    main()

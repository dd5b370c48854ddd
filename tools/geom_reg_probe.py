"""Cost of the opacity / scale / isotropy regularisers inside the backward pass (gsr_backward_args.geom_reg) at C3.

One forward pass (training form, raw parameters), then gsr_backward over and over on its buffers, alternating four cases in ONE
process, each call's preprocess_bwd stage (long_run_sums + preprocess_bwd_kernel + sh_bwd_rows_kernel + -- with the loss values --
reg_final_sum_kernel) read through gsr_profile:
  parent_null   --parent-lib, a libgsr_hip.so built from the commit before the feature: the field does not exist
  null          this tree, geom_reg = NULL: the same instructions as the parent's, so it must sit inside
                the parent's interquartile range -- the yardstick for the two below
  weights       the three weights on, loss = NULL: the REG instantiation, no extra launch
  weights_loss  weights and loss: the REG instantiation with its slab entries + the final-sum launch
Median and interquartile range of --calls calls per case behind --warmup; every case follows every other one equally often.
The pass is the unfused one (gradients written, no geom_adam): the instantiations are the same ones the fused step launches.

  python tools/geom_reg_probe.py [--calls 200] [--warmup 20] [--config C3] [--parent-lib PATH]

(Per kernel: rocprofv3 --kernel-trace --stats -- python tools/geom_reg_probe.py --calls 50, in a run of its own; the REG
instantiations carry `true` as their last template argument.)
"""
import argparse
import ctypes as C
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

RAW = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
STAGE = "preprocess_bwd"


def stage_index(lib):
    lib.gsr_profile_stage_name.restype = C.c_char_p
    lib.gsr_profile_stage_name.argtypes = [C.c_int]
    names = [lib.gsr_profile_stage_name(i).decode() for i in range(lib.gsr_profile_stage_count())]
    return names.index(STAGE), len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geom_reg_probe.py measures on the GPU: no HIP device here")
    dev = torch.device("cuda:0")
    lib = capi.load()
    cl = scene.make_config(args.config, seed=1)
    cam = cl.cameras[0]
    P = cl.xyz.shape[0]
    a = fo.inputs(cl, cam, np.zeros(3, np.float32), dev)
    a.update(opacity=fo._t(cl.opacity, dev), scales=fo._t(cl.scaling, dev), rotations=fo._t(cl.rotation, dev))
    dpix = torch.from_numpy(np.random.default_rng(0).standard_normal((3, cam.H, cam.W)).astype(np.float32)).to(dev)
    R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=RAW)
    V = max(rp.lastVisibleCount(), 1)
    grads = {n: torch.empty((P, k), device=dev) for n, k in (("dL_dopacity", 1), ("dL_dcolor", 3), ("dL_dmean3D", 3), ("dL_dsh", 48),
                                                            ("dL_dscale", 3), ("dL_drot", 4))}
    loss = torch.zeros(3, device=dev)
    scratch = torch.empty(int(lib.gsr_geom_reg_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    ba = capi.BackwardArgs()
    ba.P, ba.D, ba.M, ba.R, ba.width, ba.height = P, 3, 16, R, cam.W, cam.H
    ba.scale_modifier, ba.tan_fovx, ba.tan_fovy, ba.raw_params = 1.0, cam.tanfovx, cam.tanfovy, RAW
    for n in ("background", "means3D", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
        setattr(ba, n, a[n].data_ptr())
    ba.shs, ba.radii, ba.dL_dpix = a["sh"].data_ptr(), radii.data_ptr(), dpix.data_ptr()
    ba.geom_buffer, ba.binning_buffer, ba.image_buffer = g.data_ptr(), b.data_ptr(), i.data_ptr()
    for n, t in grads.items():
        setattr(ba, n, t.data_ptr())
    # the hosts' normalisation (MonoGS's isotropic 10, 3DGS-MCMC's 0.01 / 0.01)
    w = (0.01 / V, 0.01 / (3.0 * V), 10.0 / (3.0 * V))
    structs = {"null": None, "weights": capi.GeomReg(w[0], w[1], w[2], None, None),
               "weights_loss": capi.GeomReg(w[0], w[1], w[2], loss.data_ptr(), scratch.data_ptr())}
    libs = {k: lib for k in structs}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.gsr_backward.restype = C.c_int
        parent.gsr_backward.argtypes = [C.POINTER(capi.BackwardArgs), C.c_void_p]   # (it reads the struct up to its own last field)
        structs = dict(parent_null=None, **structs)
        libs["parent_null"] = parent
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for L in set(libs.values()):
        assert L.gsr_profile_enable(1) == 0
    idx, n_stages = stage_index(lib)
    ms = (C.c_float * n_stages)()
    times = {k: [] for k in structs}
    order = list(structs)
    for k in range(args.warmup + args.calls):
        for name in order:
            ba.geom_reg = C.pointer(structs[name]) if structs[name] is not None else None
            st = libs[name].gsr_backward(C.byref(ba), stream)
            assert st == 0, (name, st)
            assert libs[name].gsr_profile_read(ms, n_stages) == 0
            if k >= args.warmup:
                times[name].append(float(ms[idx]))
        order = order[1:] + order[:1]   # (every case follows every other one equally often)
    torch.cuda.synchronize()
    out = {"config": args.config, "P": P, "visible": V, "W": cam.W, "H": cam.H, "calls": args.calls, "stage": STAGE,
           "loss": [float(x) for x in loss.cpu()]}
    for name, t in times.items():
        q1, med, q3 = (float(np.percentile(t, q)) for q in (25, 50, 75))
        out[name] = {"median_ms": med, "q1_ms": q1, "q3_ms": q3, "iqr_ms": q3 - q1}
    if "parent_null" in out:
        out["null_inside_parent_iqr"] = bool(out["parent_null"]["q1_ms"] <= out["null"]["median_ms"] <= out["parent_null"]["q3_ms"])
    print(json.dumps(out), flush=True)
    for name in times:
        print(f"{name:13s} {out[name]['median_ms'] * 1e3:8.1f} us  (IQR {out[name]['iqr_ms'] * 1e3:.1f} us)", flush=True)


if __name__ == "__main__":
    main()

"""How the four 8x8 quads of a tile share the backward blend's visits (blend_bwd.hip), from the forward pass on the CPU emulator.

    python tools/quad_pair_probe.py [C2|C3|...] [--crop WxH] [--seed S]

Runs the product forward pass (the kernel sources compiled for the host, tests/emu) on the configuration's cloud and view, then
recomputes per (quad, list entry) what the forward blend's flags (state.h: contrib) and the backward blend's `ok` lanes hold: a
pixel blends entry e iff e < n_contrib(pixel), power <= 0 and alpha >= 1/255 (alpha with numpy's exp2: it may differ from the
device's v_exp_f32 on the rare pixel whose alpha sits on the 1/255 edge).  Prints, as JSON:
  * for each (tile, entry) some quad blends, a histogram of how many of the 4 quads blend it;
  * per pairing of the quads into two waves -- left/right (0,1)(2,3): a 16x8 half tile, top/bottom (0,2)(1,3): 8x16 -- the
    (pair, entry) visits with both quads flagged and with one, and the share of today's quad visits that fall in both-flagged pairs;
  * the mean fraction of the 64 lanes that are `ok` in a flagged quad visit.
--crop WxH keeps the configuration's focal lengths and its density of Gaussians per pixel (P scaled by the area ratio) on a
smaller image: the full C3 forward pass is slow on the emulator."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

# the package takes the emulator library only inside the test suite's runs (rasterize_points._lib): this probe is one
os.environ.setdefault("PYTEST_CURRENT_TEST", "tools/quad_pair_probe.py")

import __graft_entry__ as entry  # noqa: E402

entry.load_package()

import build_emu  # noqa: E402
import parity  # noqa: E402
from photo_slam_amd import scene  # noqa: E402

LOG2E = np.float32(1.4426950408889634)
PAIRINGS = {"left_right": ((0, 1), (2, 3)), "top_bottom": ((0, 2), (1, 3))}


def tile_flags(r, t, grid_x, W, H):
    """(flags [4][n] bool, ok counts [4][n]) of tile t's list"""
    a, b = (int(v) for v in r.ranges[t])
    n = b - a
    tx, ty = t % grid_x, t // grid_x
    ys, xs = np.mgrid[0:16, 0:16]
    px, py = tx * 16 + xs.ravel(), ty * 16 + ys.ravel()
    inside = (px < W) & (py < H)
    lc = np.zeros(256, np.int64)
    lc[inside] = r.n_contrib[py[inside], px[inside]]
    quad = ((ys.ravel() >= 8).astype(int) << 1) | (xs.ravel() >= 8).astype(int)
    flags = np.zeros((4, n), bool)
    okc = np.zeros((4, n), np.int64)
    if n == 0 or lc.max() == 0:
        return flags, okc
    m = int(lc.max())   # entries at or behind the deepest last contributor are blended by no pixel
    rec = r.rec[r.point_list[a:a + m]]
    A, B, C = (-0.5 * LOG2E * rec[:, 2]), (-LOG2E * rec[:, 3]), (-0.5 * LOG2E * rec[:, 4])
    dx = rec[:, 0:1] - px[None, :].astype(np.float32)
    dy = rec[:, 1:2] - py[None, :].astype(np.float32)
    pw = A[:, None] * dx * dx + C[:, None] * dy * dy + B[:, None] * dx * dy
    alpha = np.minimum(np.float32(0.99), rec[:, 5:6] * np.exp2(pw))
    ok = (np.arange(m)[:, None] < lc[None, :]) & ~(pw > 0) & ~(alpha < np.float32(1.0 / 255.0))
    for q in range(4):
        c = ok[:, quad == q].sum(1)
        okc[q, :m] = c
        flags[q, :m] = c > 0
    return flags, okc


def probe(config, crop=None, seed=0):
    c = scene.CONFIGS[config]
    W, H, P = c["W"], c["H"], c["P"]
    if crop:
        w, h = crop
        P = int(round(P * (w * h) / (W * H)))
        W, H = w, h
    cl = scene.make_cloud(P, W, H, c["fx"], c["fy"], seed=seed)
    cam = cl.cameras[0]
    r = parity.run_backend(build_emu.build(), torch.device("cpu"), cl, cam, np.zeros(3, np.float32), do_backward=False)
    grid_x, grid_y = (W + 15) // 16, (H + 15) // 16
    hist = np.zeros(5, np.int64)
    pair = {k: {"both": 0, "one": 0} for k in PAIRINGS}
    ok_sum, visits = 0, 0
    for t in range(grid_x * grid_y):
        f, okc = tile_flags(r, t, grid_x, W, H)
        k = f.sum(0)
        hist += np.bincount(k, minlength=5)
        for name, prs in PAIRINGS.items():
            for qa, qb in prs:
                pair[name]["both"] += int((f[qa] & f[qb]).sum())
                pair[name]["one"] += int((f[qa] ^ f[qb]).sum())
        ok_sum += int(okc[f].sum())
        visits += int(f.sum())
    out = {"config": config, "W": W, "H": H, "P": P, "seed": seed, "crop": bool(crop), "instances": int(r.R),
           "quad_visits": visits,
           "entries_by_quads_blending": {str(i): int(hist[i]) for i in range(1, 5)},
           "mean_ok_lane_fraction": ok_sum / max(visits, 1) / 64.0}
    for name in PAIRINGS:
        b, o = pair[name]["both"], pair[name]["one"]
        out[name] = {"pair_visits_both": b, "pair_visits_one": o,
                     "share_of_quad_visits_in_both_pairs": 2 * b / max(visits, 1),
                     "pair_visits_per_quad_visit": (b + o) / max(visits, 1)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C2")
    ap.add_argument("--crop", default=None, help="WxH")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    crop = tuple(int(v) for v in a.crop.split("x")) if a.crop else None
    print(json.dumps(probe(a.config, crop, a.seed), indent=1))

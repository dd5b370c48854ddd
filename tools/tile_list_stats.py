"""Per-tile list statistics of a bench config on the CPU, from numpy alone (the projection and rectangle rule of csrc/preprocess.hip
on scene.make_config(name, seed=0)): list lengths, key spans, and the runs of equal 18-bit prefix of key - min that the fix-up of
csrc/tile_depth_sort.hip ranks -- how many lists would fall back to the exact passes at a given TDS_CAP (EXPERIMENTS section R8).

  python tools/tile_list_stats.py C3 C2        (prints to stdout)

float32 throughout, in the kernel's operation order; numpy rounds a few products differently from the device's unfused arithmetic
(C3: 6 237 786 instances against the device's 6 237 787).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from photo_slam_amd import scene  # noqa: E402

f32 = np.float32
TILE = 16
PREFIX_BITS = 18   # two 9-bit passes of tile_depth_sort.hip


def f2i(a):
    """preprocess.hip: f2i (NaN -> 0, saturating truncation)"""
    a = np.where(np.isnan(a), 0, a)
    return np.trunc(np.clip(a, -2147483648.0, 2147483647.0)).astype(np.int64)


def cov3d(cl):
    """kernels.h: compute_cov3D on the activated scales and rotations"""
    s = cl.get_scaling()
    q = cl.get_rotation()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f32(1), f32(2)
    R00 = one - two * (y * y + z * z)
    R01 = two * (x * y - r * z)
    R02 = two * (x * z + r * y)
    R10 = two * (x * y + r * z)
    R11 = one - two * (x * x + z * z)
    R12 = two * (y * z - r * x)
    R20 = two * (x * z - r * y)
    R21 = two * (y * z + r * x)
    R22 = one - two * (x * x + y * y)
    s0, s1, s2 = s[:, 0], s[:, 1], s[:, 2]
    M00, M01, M02 = s0 * R00, s1 * R01, s2 * R02
    M10, M11, M12 = s0 * R10, s1 * R11, s2 * R12
    M20, M21, M22 = s0 * R20, s1 * R21, s2 * R22
    return [M00 * M00 + M01 * M01 + M02 * M02,
            M10 * M00 + M11 * M01 + M12 * M02,
            M20 * M00 + M21 * M01 + M22 * M02,
            M10 * M10 + M11 * M11 + M12 * M12,
            M20 * M10 + M21 * M11 + M22 * M12,
            M20 * M20 + M21 * M21 + M22 * M22]


def project(cl, cam, W, H):
    """preprocess.hip, phase 1: per Gaussian its depth key, tile rectangle and whether it is visible"""
    xyz = cl.xyz.astype(f32)
    V = cam.viewmatrix.astype(f32).reshape(-1)
    Pm = cam.projmatrix.astype(f32).reshape(-1)
    px, py, pz = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    vz = V[2] * px + V[6] * py + V[10] * pz + V[14]
    ok = vz > f32(0.2)
    hx = Pm[0] * px + Pm[4] * py + Pm[8] * pz + Pm[12]
    hy = Pm[1] * px + Pm[5] * py + Pm[9] * pz + Pm[13]
    hw = Pm[3] * px + Pm[7] * py + Pm[11] * pz + Pm[15]
    p_w = f32(1.0) / (hw + f32(0.0000001))
    projx, projy = hx * p_w, hy * p_w
    c3 = cov3d(cl)
    tx = V[0] * px + V[4] * py + V[8] * pz + V[12]
    ty = V[1] * px + V[5] * py + V[9] * pz + V[13]
    with np.errstate(all="ignore"):   # (culled Gaussians divide by depths near zero)
        tz = vz
        limx = f32(1.3) * f32(cam.tanfovx)
        limy = f32(1.3) * f32(cam.tanfovy)
        tx = np.minimum(limx, np.maximum(-limx, tx / tz)) * tz
        ty = np.minimum(limy, np.maximum(-limy, ty / tz)) * tz
        focal_x = f32(W / (2 * cam.tanfovx))
        focal_y = f32(H / (2 * cam.tanfovy))
        J00, J02 = focal_x / tz, -(focal_x * tx) / (tz * tz)
        J11, J12 = focal_y / tz, -(focal_y * ty) / (tz * tz)
        T00, T01, T02 = V[0] * J00 + V[2] * J02, V[4] * J00 + V[6] * J02, V[8] * J00 + V[10] * J02
        T10, T11, T12 = V[1] * J11 + V[2] * J12, V[5] * J11 + V[6] * J12, V[9] * J11 + V[10] * J12
        A00 = T00 * c3[0] + T01 * c3[1] + T02 * c3[2]
        A10 = T00 * c3[1] + T01 * c3[3] + T02 * c3[4]
        A20 = T00 * c3[2] + T01 * c3[4] + T02 * c3[5]
        A01 = T10 * c3[0] + T11 * c3[1] + T12 * c3[2]
        A11 = T10 * c3[1] + T11 * c3[3] + T12 * c3[4]
        A21 = T10 * c3[2] + T11 * c3[4] + T12 * c3[5]
        cov00 = (A00 * T00 + A10 * T01 + A20 * T02) + f32(0.3)
        cov01 = A01 * T00 + A11 * T01 + A21 * T02
        cov11 = (A01 * T10 + A11 * T11 + A21 * T12) + f32(0.3)
        det = cov00 * cov11 - cov01 * cov01
        ok &= det != 0
        mid = f32(0.5) * (cov00 + cov11)
        root = np.sqrt(np.maximum(f32(0.1), mid * mid - det))
        radius = np.ceil(f32(3) * np.sqrt(np.maximum(mid + root, mid - root)))
        pix = (((projx.astype(np.float64) + 1.0) * W - 1.0) * 0.5).astype(f32)
        piy = (((projy.astype(np.float64) + 1.0) * H - 1.0) * 0.5).astype(f32)
        grid_x, grid_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        mr = f2i(radius).astype(f32)
        T = f32(TILE)
        rminx = np.clip(f2i((pix - mr) / T), 0, grid_x)
        rminy = np.clip(f2i((piy - mr) / T), 0, grid_y)
        rmaxx = np.clip(f2i((pix + mr + f32(TILE - 1)) / T), 0, grid_x)
        rmaxy = np.clip(f2i((piy + mr + f32(TILE - 1)) / T), 0, grid_y)
    ok &= (rmaxy - rminy) * (rmaxx - rminx) > 0
    return vz.view(np.uint32), (rminx, rminy, rmaxx, rmaxy), ok, grid_x


def tile_lists(key, rect, ok, grid_x):
    """the (tile, key) of every instance, sorted by tile and then key; the first index and the length of every tile's list"""
    rminx, rminy, rmaxx, rmaxy = rect
    ids = np.nonzero(ok)[0]
    w = (rmaxx - rminx)[ids]
    h = (rmaxy - rminy)[ids]
    n = w * h
    rep = np.repeat(np.arange(len(ids)), n)
    off = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    tile = (rminy[ids][rep] + off // w[rep]) * grid_x + rminx[ids][rep] + off % w[rep]
    k = key[ids][rep].astype(np.int64)
    order = np.lexsort((k, tile))
    tile, k = tile[order], k[order]
    starts = np.nonzero(np.r_[True, tile[1:] != tile[:-1]])[0]
    lens = np.diff(np.r_[starts, len(tile)])
    return len(ids), tile, k, starts, lens


def run(name):
    cl = scene.make_config(name, seed=0)
    c = scene.CONFIGS[name]
    key, rect, ok, grid_x = project(cl, cl.cameras[0], c["W"], c["H"])
    visible, tile, k, starts, lens = tile_lists(key, rect, ok, grid_x)
    print(name, "visible", visible, "instances", len(k))
    print(" lists", len(lens), "mean", lens.mean(), "median", np.median(lens), "p99", np.percentile(lens, 99), "max", lens.max(),
          "over 2048:", int((lens > 2048).sum()))
    kmin = np.minimum.reduceat(k, starts)
    span = np.maximum.reduceat(k, starts) - kmin
    bits = np.where(span > 0, np.floor(np.log2(np.maximum(span, 1))).astype(int) + 1, 0)
    print(" bits hist", dict(zip(*np.unique(bits, return_counts=True))))
    fixup = (lens <= 2048) & (bits > PREFIX_BITS) & (bits <= PREFIX_BITS + 9)   # the lists that take two passes + fix-up
    print(" in-LDS tiles with 19..27 bits:", int(fixup.sum()), "of", len(lens))
    low = np.repeat(np.maximum(bits - PREFIX_BITS, 0), lens)
    prefix = (k - np.repeat(kmin, lens)) >> low
    run_starts = np.nonzero(np.r_[True, (prefix[1:] != prefix[:-1]) | (tile[1:] != tile[:-1])])[0]
    run_lens = np.diff(np.r_[run_starts, len(k)])
    run_tile = np.searchsorted(starts, run_starts, side="right") - 1
    longest = np.zeros(len(lens), int)
    np.maximum.at(longest, run_tile, run_lens)
    shared = np.zeros(len(lens), int)
    np.add.at(shared, run_tile, (run_lens > 1).astype(int))
    print(" runs of >1 per in-LDS 3-pass tile: mean", shared[fixup].mean(), "max run hist",
          dict(zip(*np.unique(longest[fixup], return_counts=True))))
    for cap in (2, 3, 4, 6, 8, 12, 16):
        fallback = int((longest[fixup] > cap).sum())
        print(f" CAP {cap}: fallback tiles {fallback} ({100.0 * fallback / max(fixup.sum(), 1):.3f} %)")


if __name__ == "__main__":
    for config in sys.argv[1:] or ["C3", "C2"]:
        run(config)

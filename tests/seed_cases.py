"""Shared checks of the seeding kernels (gsr_seed_select, gsr_seed_emit; include/gsr.h) and of the hosts' seedFromDepth, run by
test_seed.py on the emulator build, by test_gpu_seed.py on the MI355X and by test_cpp_host_seed.py for the C++ host.

Every reference here is numpy written from the definitions in include/gsr.h: float32 for the comparisons (the selection, its order,
the counts and the median's bits are checked as integers, no tolerance), float64 for the values of a written row (bar BAR_VALUES; how
it was set is written in the docstrings of the two test files)."""
import copy
import ctypes as C
import math

import numpy as np
import torch

from photo_slam_amd import capi, scene

f32 = np.float32
# (W, H): one pixel, the wave boundaries, one tile of 1024 pixels and its boundary, odd sizes that are no multiple of the four pixels
# a thread owns, several tiles
SIZES = [(1, 1), (63, 1), (64, 1), (65, 1), (16, 16), (257, 1), (33, 31), (41, 25), (229, 131)]
GPU_ONLY_SIZE = (640, 411)           # 263 040 pixels: the first size past 1024 groups of 256 pixels
PAST_ONE_CHUNK = (1025, 1024)        # 1 049 600 pixels: the first size past one chunk of the spine scan (1024 tile totals of 1024 pixels)
HOST_SIZE = (229, 131)

# the next power of ten above ten times the larger of the emulator's and the MI355X's largest relative error (test_seed.py and
# test_gpu_seed.py carry the two measurements)
BAR_VALUES = 1e-5

NAMES = ("xyz", "features", "opacity", "scaling", "rotation")
C0 = float(f32(0.28209479177387814))
DEFAULTS = dict(min_depth=0.3, max_depth=6.0, alpha_threshold=0.5, depth_error_abs=0.0, depth_error_median_factor=3.0, stride=1,
                offset_x=0, offset_y=0)


def camera(W, H):
    """a rigid pose that is not the identity; fx, fy, cx, cy of the rasterizer's pixel-centre convention"""
    cam = scene.make_camera(W, H, 0.9 * max(W, 8), 0.8 * max(W, 8), scene.look_rotation(0.7, 0.2), np.array([0.3, -0.2, 1.1]))
    return dict(viewmatrix=cam.viewmatrix.astype(f32), fx=f32(W / (2.0 * cam.tanfovx)), fy=f32(H / (2.0 * cam.tanfovy)),
                cx=f32((W - 1) / 2.0), cy=f32((H - 1) / 2.0))


def make_maps(W, H, seed=0, kind="mixed"):
    """gt depth in [0.5, 5] with, where the image is large enough, pixels of 0, NaN, inf, min_depth and max_depth exactly; alpha in
    [0, 1] on both sides of the threshold; depth = gt + an error, the error mostly small and for about a tenth of the
    pixels large and in front.  kind: 'mixed', 'none' (alpha 1, depth = gt: nothing selected), 'all' (alpha 0), 'equal' (every error
    the same)."""
    rng = np.random.default_rng(seed)
    n = W * H
    gt = rng.uniform(0.5, 5.0, n).astype(f32)
    alpha = rng.uniform(0.0, 1.0, n).astype(f32)
    err = rng.normal(0.0, 0.01, n).astype(f32)
    big = rng.random(n) < 0.1
    err[big] = rng.uniform(0.5, 2.0, int(big.sum())).astype(f32)
    depth = (gt + err).astype(f32)
    depth[rng.random(n) < 0.05] *= f32(0.5)   # (behind: never selected by the depth rule)
    if kind == "none":
        alpha[:] = 1.0
        depth = gt.copy()
    elif kind == "all":
        alpha[:] = 0.0
    elif kind == "equal":
        gt = (np.round(gt * f32(1024.0)) / f32(1024.0)).astype(f32)   # (multiples of 2^-10 below 8: gt + 0.25 is exact)
        depth = (gt + f32(0.25)).astype(f32)
    if n >= 16 and kind != "equal":
        bad = rng.choice(n, 5, replace=False)
        gt[bad] = np.array([0.0, np.nan, np.inf, DEFAULTS["min_depth"], DEFAULTS["max_depth"]], f32)
    image = rng.uniform(0.0, 1.0, (3, H, W)).astype(f32)
    return dict(W=W, H=H, gt=gt.reshape(H, W), alpha=alpha.reshape(H, W), depth=depth.reshape(H, W), image=image)


def reference_select(m, o, maps=True):
    """the definition in float32: (selected pixels in row-major order, counts[0..4], T)"""
    W, H = m["W"], m["H"]
    g = m["gt"].reshape(-1).astype(f32)
    a = m["alpha"].reshape(-1).astype(f32) if maps else np.zeros(W * H, f32)
    d = m["depth"].reshape(-1).astype(f32) if maps else np.zeros(W * H, f32)
    with np.errstate(invalid="ignore"):
        valid = (g > f32(o["min_depth"])) & (g < f32(o["max_depth"]))
        e = np.abs(g - d).astype(f32)
        n_valid = int(valid.sum())
        absT, factor = f32(o["depth_error_abs"]), f32(o["depth_error_median_factor"])
        med = f32(0.0)
        if factor != 0 and n_valid:
            k = (n_valid - 1) // 2
            med = np.partition(e[valid], k)[k]
        T = np.maximum(absT, f32(factor * med)) if factor != 0 else absT
        rule = factor != 0 or absT != 0
        in_front = (d > g) & (e > T) if rule else np.zeros(W * H, bool)
        unseen = a < f32(o["alpha_threshold"])
    p = np.arange(W * H)
    u, v = p % W, p // W
    cand = (u % o["stride"] == o["offset_x"]) & (v % o["stride"] == o["offset_y"])
    sel = cand & valid & (unseen | in_front)
    med_bits = int(np.array([med], f32).view(np.uint32)[0]) if (factor != 0 and n_valid) else 0
    counts = [int(sel.sum()), int((sel & unseen).sum()), int((sel & ~unseen).sum()), n_valid, med_bits]
    return np.flatnonzero(sel), counts, T


def thinning(n_selected, n_emit):
    """(the ranks written, the rows they go to): the uint64 formula of the header"""
    r = np.arange(n_selected, dtype=np.uint64)
    lo = r * np.uint64(n_emit) // np.uint64(n_selected)
    hi = (r + np.uint64(1)) * np.uint64(n_emit) // np.uint64(n_selected)
    keep = hi > lo
    return np.flatnonzero(keep), lo[keep].astype(np.int64)


def make_rows(P, room, M=4, seed=0):
    """P live rows with recognisable values and `room` rows behind them filled with a sentinel (every array, the moments too)"""
    rng = np.random.default_rng(seed + 77)
    n = P + room
    d = {}
    shapes = dict(xyz=(n, 3), features=(n, M, 3), opacity=(n, 1), scaling=(n, 3), rotation=(n, 4))
    for name in NAMES:
        d[name] = rng.normal(size=shapes[name]).astype(f32)
        d["m1_" + name] = rng.normal(size=shapes[name]).astype(f32)
        d["m2_" + name] = (rng.random(size=shapes[name]) + 0.5).astype(f32)
    d["exist"] = rng.integers(1, 1000, size=n).astype(np.int32)
    for k in range(3):
        d[f"stat{k}"] = (rng.random(n) + 1.0).astype(f32)
    for k, v in d.items():
        v[P:] = 777 if v.dtype == np.int32 else f32(-123.5)
    return d


def _dev_tensor(a, dev, misalign=False):
    """misalign: the data starts 4 bytes past a 16-byte boundary (the 4-byte load path of gsr_seed_select)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def select(lib_path, dev, m, o, maps=True, misalign=False, status_only=False, raw=None):
    lib = capi.load(lib_path)
    t = {k: _dev_tensor(m[k], dev, misalign) for k in ("gt", "alpha", "depth")}
    a = capi.SeedSelectArgs()
    a.width, a.height = m["W"], m["H"]
    a.gt_depth = t["gt"].data_ptr()
    if maps:
        a.alpha, a.depth = t["alpha"].data_ptr(), t["depth"].data_ptr()
    for k in ("min_depth", "max_depth", "alpha_threshold", "depth_error_abs", "depth_error_median_factor", "stride", "offset_x", "offset_y"):
        setattr(a, k, o[k])
    for k, v in (raw or {}).items():
        setattr(a, k, v)
    scratch = torch.empty(int(lib.gsr_seed_scratch_bytes(m["W"], m["H"])) + 256, dtype=torch.uint8, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream if dev.type != "cpu" else None
    st = lib.gsr_seed_select(C.byref(a), scratch.data_ptr(), counts.data_ptr(), stream)
    if dev.type != "cpu":
        torch.cuda.synchronize()
    return st, counts.cpu().numpy(), scratch, t


def emit(lib_path, dev, m, o, cam, scratch, gt_t, n_selected, n_emit, d, P, iteration=41, scale_factor=1.5, init_opacity=0.3,
         moments=True, extras=True, image=True, raw=None):
    """gsr_seed_emit on copies of d's arrays; returns (status, arrays after, out_pixel)"""
    lib = capi.load(lib_path)
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in d.items()}
    img = torch.from_numpy(m["image"]).to(dev)
    vm = torch.from_numpy(cam["viewmatrix"]).to(dev).contiguous()
    pix = torch.full((max(n_emit, 1) + 3,), -5, dtype=torch.int32, device=dev)
    e = capi.SeedEmitArgs()
    e.width, e.height, e.stride, e.n_selected, e.n_emit, e.P = m["W"], m["H"], o["stride"], n_selected, n_emit, P
    e.features_row_floats = int(d["features"].shape[1] * d["features"].shape[2])
    e.gt_depth, e.image, e.viewmatrix = gt_t.data_ptr(), (img.data_ptr() if image else None), vm.data_ptr()
    e.fx, e.fy, e.cx, e.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    e.scale_factor, e.init_opacity, e.iteration = scale_factor, init_opacity, iteration
    for i, name in enumerate(NAMES):
        e.param[i] = t[name].data_ptr()
        if moments:
            e.exp_avg[i], e.exp_avg_sq[i] = t["m1_" + name].data_ptr(), t["m2_" + name].data_ptr()
    if extras:
        e.exist_since_iter = t["exist"].data_ptr()
        for k in range(3):
            e.stats[k] = t[f"stat{k}"].data_ptr()
    e.out_pixel = pix.data_ptr()
    sp = scratch.data_ptr()
    for k, v in (raw or {}).items():
        if k == "scratch":
            sp = v
        elif isinstance(v, tuple):
            getattr(e, k)[v[0]] = v[1]
        else:
            setattr(e, k, v)
    stream = torch.cuda.current_stream().cuda_stream if dev.type != "cpu" else None
    st = lib.gsr_seed_emit(C.byref(e), sp, stream)
    if dev.type != "cpu":
        torch.cuda.synchronize()
    return st, {k: v.cpu().numpy() for k, v in t.items()}, pix.cpu().numpy()


def reference_rows(m, cam, pixels, stride, scale_factor, init_opacity, M, image=True):
    """the values of the rows written for `pixels`, float64, from the float32 inputs"""
    W = m["W"]
    px = np.asarray(pixels, np.int64)
    u, v = (px % W).astype(np.float64), (px // W).astype(np.float64)
    z = m["gt"].reshape(-1)[px].astype(np.float64)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    vm = cam["viewmatrix"].astype(np.float64).reshape(-1)          # element (r, c) at [4c + r]
    R = np.array([[vm[4 * c + r] for c in range(3)] for r in range(3)])
    t = vm[12:15]
    xyz = (pc - t) @ R                                            # R^T (p_c - t), row-wise
    scaling = np.log(float(f32(scale_factor)) * stride * z / (0.5 * (fx + fy)))
    feat = np.zeros((len(px), M, 3))
    if image:
        feat[:, 0, :] = (m["image"].reshape(3, -1)[:, px].T.astype(np.float64) - 0.5) / C0
    o = float(f32(init_opacity))
    return dict(xyz=xyz, scaling=np.repeat(scaling[:, None], 3, 1), features=feat, opacity=np.full((len(px), 1), math.log(o / (1.0 - o))),
                xyz_scale=np.maximum(np.abs(pc).max(1), np.abs(t).max())[:, None])


def check_case(lib_path, dev, W, H, seed=0, kind="mixed", maps=True, n_emit="all", M=4, P=5, moments=True, extras=True, image=True,
               misalign=False, m=None, **opts):
    """select + emit against the definition.  n_emit: 'all', an integer, or a function of n_selected.  Returns (the largest relative
    error of the written values, counts, out_pixel)."""
    o = dict(DEFAULTS, **opts)
    m = make_maps(W, H, seed, kind) if m is None else m
    cam = camera(W, H)
    st, counts, scratch, t = select(lib_path, dev, m, o, maps=maps, misalign=misalign)
    assert st == 0, st
    want_pix, want_counts, T = reference_select(m, o, maps)
    assert list(counts[:5].view(np.uint32)) == want_counts, (counts, want_counts)
    assert np.all(counts[5:] == 0)
    n_sel = want_counts[0]
    n = n_sel if n_emit == "all" else (n_emit(n_sel) if callable(n_emit) else n_emit)
    n = max(0, min(n, n_sel))
    tail = 3
    d = make_rows(P, n + tail, M=M, seed=seed)
    st, out, pix = emit(lib_path, dev, m, o, cam, scratch, t["gt"], n_sel, n, d, P, moments=moments, extras=extras, image=image)
    assert st == 0, st
    # ---- which pixels, in which rows: integers
    if n:
        ranks, rows = thinning(n_sel, n)
        assert len(ranks) == n and np.array_equal(rows, np.arange(n))
        want_rows_pix = want_pix[ranks]
    else:
        want_rows_pix = np.zeros(0, np.int64)
    assert np.array_equal(pix[:n], want_rows_pix), (pix[:8], want_rows_pix[:8])
    assert np.all(pix[n:] == -5), "out_pixel written past n_emit"
    if n_emit == "all":
        assert np.array_equal(pix[:n], want_pix), "not the selection in row-major order"
    # ---- nothing outside [P, P + n)
    new = slice(P, P + n)
    for k, v in d.items():
        assert np.array_equal(out[k][:P].view(np.uint32), v[:P].view(np.uint32)), f"{k}: a live row changed"
        assert np.array_equal(out[k][P + n:].view(np.uint32), v[P + n:].view(np.uint32)), f"{k}: the room behind the new rows changed"
    # ---- moments, statistics, exist_since_iter of the new rows
    for name in NAMES:
        for mm in ("m1_", "m2_"):
            if moments:
                assert np.all(out[mm + name][new].view(np.uint32) == 0), f"{mm}{name}: not exactly zero in a new row"
            else:
                assert np.array_equal(out[mm + name].view(np.uint32), d[mm + name].view(np.uint32))
    if extras:
        assert np.all(out["exist"][new] == 41)
        for k in range(3):
            assert np.all(out[f"stat{k}"][new].view(np.uint32) == 0)
    else:
        assert np.array_equal(out["exist"], d["exist"]) and all(np.array_equal(out[f"stat{k}"], d[f"stat{k}"]) for k in range(3))
    # ---- the values
    worst = 0.0
    if n:
        ref = reference_rows(m, cam, want_rows_pix, o["stride"], 1.5, 0.3, M, image=image)
        assert np.array_equal(out["rotation"][new], np.tile(np.array([1, 0, 0, 0], f32), (n, 1)))
        feat = out["features"][new].astype(np.float64)
        assert np.all(feat[:, 1:, :] == 0), "the SH row behind the DC term is not zero"
        errs = [np.abs(out["xyz"][new] - ref["xyz"]) / ref["xyz_scale"],
                np.abs(out["scaling"][new] - ref["scaling"]) / np.maximum(1.0, np.abs(ref["scaling"])),
                np.abs(feat[:, 0, :] - ref["features"][:, 0, :]) / np.maximum(1.0, np.abs(ref["features"][:, 0, :])),
                np.abs(out["opacity"][new] - ref["opacity"]) / np.maximum(1.0, np.abs(ref["opacity"]))]
        worst = float(max(e.max() for e in errs))
        print(f"measured: {W}x{H} xyz / scaling / DC / logit, largest relative errors:", [float(e.max()) for e in errs])
        assert worst <= BAR_VALUES, worst
        assert len(np.unique(out["opacity"][new].view(np.uint32))) == 1
        sc_bits = out["scaling"][new].view(np.uint32)
        assert np.array_equal(sc_bits[:, 0], sc_bits[:, 1]) and np.array_equal(sc_bits[:, 0], sc_bits[:, 2]), "the three scales differ"
    return worst, counts, pix[:n]


def check_median(lib_path, dev):
    """the median's bits against np.partition: odd and even numbers of valid pixels, and every error equal"""
    for W, H, seed in ((33, 31, 1), (41, 25, 2), (257, 1, 3), (16, 16, 4)):
        m = make_maps(W, H, seed)
        n_valid = reference_select(m, DEFAULTS)[1][3]
        for drop in (0, 1):   # one more invalid pixel flips the parity
            if drop:
                m["gt"].reshape(-1)[np.flatnonzero(np.isfinite(m["gt"].reshape(-1)) & (m["gt"].reshape(-1) > 1))[0]] = 0.0
            _, counts, _ = check_case(lib_path, dev, W, H, m=m)
            assert counts[4] != 0
        assert reference_select(m, DEFAULTS)[1][3] == n_valid - 1
    _, counts, _ = check_case(lib_path, dev, 41, 25, kind="equal", seed=5)
    assert counts[4] == int(np.array([0.25], f32).view(np.uint32)[0]) and counts[0] > 0
    # the median alone decides: a factor that puts T just below and just above the large errors
    for factor in (1.0, 1e4):
        check_case(lib_path, dev, 33, 31, seed=6, depth_error_median_factor=factor)


def check_strides(lib_path, dev):
    for stride, (W, H) in ((1, (41, 25)), (2, (41, 25)), (3, (41, 25)), (8, (33, 31))):
        total = 0
        for oy in range(stride):
            for ox in range(stride):
                _, counts, _ = check_case(lib_path, dev, W, H, seed=7, stride=stride, offset_x=ox, offset_y=oy)
                total += counts[0]
        assert total == reference_select(make_maps(W, H, 7), DEFAULTS)[1][0], "the offsets of a stride do not partition the selection"


def check_thinning(lib_path, dev, W=41, H=25):
    for n_emit in (1, lambda s: s - 1, lambda s: s // 3):
        check_case(lib_path, dev, W, H, seed=8, n_emit=n_emit)
    check_case(lib_path, dev, W, H, seed=8, n_emit=0)


def check_corners(lib_path, dev):
    _, counts, _ = check_case(lib_path, dev, 41, 25, kind="none", seed=9)
    assert counts[0] == 0
    m = make_maps(41, 25, 10, "all")
    _, counts, _ = check_case(lib_path, dev, 41, 25, m=m)
    assert counts[0] == counts[3] == counts[1] > 0
    m["gt"][:] = np.clip(m["gt"], 0.5, 5.0)
    m["gt"][~np.isfinite(m["gt"])] = 1.0
    _, counts, _ = check_case(lib_path, dev, 41, 25, m=m)
    assert counts[0] == 41 * 25, "everything selected"
    # alpha and depth NULL: every valid candidate is unseen; the median is that of gt itself
    _, counts, _ = check_case(lib_path, dev, 33, 31, seed=11, maps=False)
    assert counts[0] == counts[3] and counts[2] == 0
    # the invalid values: 0, NaN, inf, min_depth exactly, max_depth exactly are in make_maps; none of them is selected
    m = make_maps(33, 31, 12)
    _, counts, pix = check_case(lib_path, dev, 33, 31, m=m, alpha_threshold=2.0)
    g = m["gt"].reshape(-1)
    assert counts[0] == 33 * 31 - 5 and np.all(np.isfinite(g[pix])) and np.all((g[pix] > DEFAULTS["min_depth"]) & (g[pix] < DEFAULTS["max_depth"]))
    # max_depth = inf: inf still fails
    _, counts, _ = check_case(lib_path, dev, 33, 31, m=m, alpha_threshold=2.0, max_depth=float("inf"), min_depth=0.0)
    assert counts[0] == 33 * 31 - 3
    # the depth rule off, and abs only
    _, c_off, _ = check_case(lib_path, dev, 33, 31, seed=13, depth_error_abs=0.0, depth_error_median_factor=0.0)
    assert c_off[2] == 0 and c_off[4] == 0
    _, c_abs, _ = check_case(lib_path, dev, 33, 31, seed=13, depth_error_abs=0.4, depth_error_median_factor=0.0)
    assert c_abs[2] > 0 and c_abs[4] == 0
    # abs above factor * median
    _, c_both, _ = check_case(lib_path, dev, 33, 31, seed=13, depth_error_abs=0.4, depth_error_median_factor=1.0)
    assert c_both[2] == c_abs[2] and c_both[4] != 0
    # other SH rows, no moments, no extras, no image, maps off a 16-byte boundary
    check_case(lib_path, dev, 33, 31, seed=14, M=1)
    check_case(lib_path, dev, 33, 31, seed=14, M=16, P=0)
    check_case(lib_path, dev, 33, 31, seed=14, moments=False, extras=False, image=False)
    check_case(lib_path, dev, 229, 131, seed=14, misalign=True)


def check_determinism(lib_path, dev, W=229, H=131):
    m = make_maps(W, H, 15)
    cam = camera(W, H)
    runs = []
    for _ in range(2):
        st, counts, scratch, t = select(lib_path, dev, m, DEFAULTS)
        n = int(counts[0])
        st2, out, pix = emit(lib_path, dev, m, DEFAULTS, cam, scratch, t["gt"], n, n // 2, make_rows(3, n // 2), 3)
        assert st == 0 and st2 == 0
        runs.append((counts, out, pix))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k].view(np.uint32), runs[1][1][k].view(np.uint32)), k


def check_api_contract(lib_path, dev):
    lib = capi.load(lib_path)
    INVALID = -1
    m = make_maps(16, 16, 0)
    cam = camera(16, 16)
    ok = select(lib_path, dev, m, DEFAULTS)
    assert ok[0] == 0
    for raw in (dict(stride=0), dict(stride=-1), dict(stride=2, offset_x=2), dict(stride=2, offset_y=-1), dict(offset_x=1), dict(alpha=None),
                dict(depth=None), dict(gt_depth=None), dict(width=-1)):
        assert select(lib_path, dev, m, DEFAULTS, raw=raw)[0] == INVALID, raw
    assert lib.gsr_seed_select(None, None, None, None) == INVALID
    st, counts, _, _ = select(lib_path, dev, m, DEFAULTS, raw=dict(width=0))
    assert st == 0 and list(counts) == [0] * 8
    st, counts, _, _ = select(lib_path, dev, m, DEFAULTS, raw=dict(height=0))
    assert st == 0 and list(counts) == [0] * 8
    assert lib.gsr_seed_scratch_bytes(0, 0) > 0 and lib.gsr_seed_scratch_bytes(1920, 1080) > lib.gsr_seed_scratch_bytes(64, 64)
    assert lib.gsr_seed_scratch_bytes(-3, 5) == lib.gsr_seed_scratch_bytes(0, 0)
    _, counts, scratch, t = ok
    n = int(counts[0])
    assert n > 2
    d = make_rows(4, n)

    def status(**raw):
        st, out, _ = emit(lib_path, dev, m, DEFAULTS, cam, scratch, t["gt"], n, n, d, 4, raw=raw)
        return st, out
    assert status()[0] == 0
    for raw in (dict(stride=0), dict(init_opacity=0.0), dict(init_opacity=1.0), dict(init_opacity=-0.2), dict(init_opacity=float("nan")),
                dict(n_emit=n + 1), dict(n_emit=-1), dict(n_selected=-1), dict(P=-1), dict(param=(0, None)), dict(param=(3, None)),
                dict(exp_avg=(2, None)), dict(exp_avg_sq=(4, None)), dict(features_row_floats=0), dict(gt_depth=None),
                dict(viewmatrix=None), dict(scratch=None), dict(width=-1)):
        assert status(**raw)[0] == INVALID, raw
    assert lib.gsr_seed_emit(None, None, None) == INVALID
    for raw in (dict(n_emit=0), dict(width=0), dict(height=0)):   # nothing is written
        st, out = status(**raw)
        assert st == 0, raw
        for k in d:
            assert np.array_equal(out[k].view(np.uint32), d[k].view(np.uint32)), (raw, k)


# ------------------------------------------------------------------------------------------------------------ the hosts
def _host_modules():
    import geom_reg_cases as gr
    from photo_slam_amd import rasterize_points as rp
    return gr, rp


HOST_P = 4000
_host = {}


def host_scene():
    """the project's generated scene at 229 x 131; the rows whose means project into the central rectangle"""
    if "cl" not in _host:
        gr, _ = _host_modules()
        W, H = HOST_SIZE
        cl = gr.cloud(HOST_P, seed=6, scale_k=0.15, size=(W, H, 150.0))
        cam = cl.cameras[0]
        h = np.concatenate([cl.xyz.astype(np.float64), np.ones((HOST_P, 1))], 1) @ cam.projmatrix.astype(np.float64)
        px = ((h[:, 0] / h[:, 3] + 1.0) * W - 1.0) * 0.5
        py = ((h[:, 1] / h[:, 3] + 1.0) * H - 1.0) * 0.5
        rect = (W // 4, H // 4, 3 * W // 4, 3 * H // 4)
        inside = (h[:, 3] > 0) & (px >= rect[0]) & (px < rect[2]) & (py >= rect[1]) & (py < rect[3])
        _host.update(cl=cl, inside=inside, rect=rect)
    return copy.deepcopy(_host["cl"]), _host["inside"].copy(), _host["rect"]


def python_trainer(cl, dev, **attrs):
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev) if cl is not None else GaussianModel(3, dev)
    opt = GaussianOptimizationParams()
    opt.lambda_dssim_ = 0.0
    if cl is not None:
        g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent) if cl is not None else 1.0,
                   seed=7)
    ts.depth_min_, ts.depth_max_ = 0.1, 100.0
    for k, v in attrs.items():
        setattr(ts, k, v)
    return g, ts


def host_frame(dev):
    """(cloud, keyframe, gt image, gt depth = the full model's depth / alpha, mask of the rows to prune, rectangle)"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl, inside, rect = host_scene()
    kf = GaussianKeyframe.from_camera(cl.cameras[0], dev)
    g, ts = python_trainer(cl, dev)
    image, depth, alpha = ts.render_view(kf, with_depth=True)
    return cl, kf, image.clone(), (depth / alpha).clone(), torch.from_numpy(inside).to(dev), rect


def _ts_options(ts):
    return dict(min_depth=ts.depth_min_, max_depth=ts.depth_max_, alpha_threshold=ts.seed_alpha_threshold_,
                depth_error_abs=ts.seed_depth_error_abs_, depth_error_median_factor=ts.seed_depth_median_factor_,
                stride=ts.seed_stride_, offset_x=0, offset_y=0)


def _maps_of(ts, kf, gt_depth):
    W, H = kf.image_width_, kf.image_height_
    _, depth, alpha = ts.render_view(kf, with_depth=True)
    return dict(W=W, H=H, gt=gt_depth.cpu().numpy(), alpha=alpha.cpu().numpy(), depth=depth.cpu().numpy())


def check_host_python(lib_path, dev):
    """seedFromDepth on the pruned scene: exactly the rows the numpy rule selects from the host's own render, where the map's alpha
    was low or the depth rule fired; the hole fills; a second call selects what the rule selects on the new maps; a seed rendered
    alone lands on its pixel.  Returns (first count, second count)."""
    gr, rp = _host_modules()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, kf, gt_image, gt_depth, inside, rect = host_frame(dev)
        W, H = kf.image_width_, kf.image_height_
        g, ts = python_trainer(cl, dev)
        g.prunePoints(inside)
        P = int(g.xyz_.shape[0])
        assert 0 < P < HOST_P
        m0 = _maps_of(ts, kf, gt_depth)
        want_pix, want_counts, T = reference_select(m0, _ts_options(ts))
        print(f"measured: {HOST_P - P} of {HOST_P} rows pruned; the rule selects {want_counts} (T = {T}); mean alpha of the pruned map {m0['alpha'].mean()}")
        sparse = (g.sparse_points_xyz_, g.sparse_points_color_)
        n = ts.seedFromDepth(kf, gt_image, gt_depth, 17, want_pixels=True)
        assert n == want_counts[0] > 0 and g.last_seed_counts_ == want_counts, (n, g.last_seed_counts_, want_counts)
        pix = g.last_seed_pixels_.cpu().numpy()
        assert np.array_equal(pix, want_pix)
        assert (g.sparse_points_xyz_, g.sparse_points_color_) == sparse
        for t in g.params() + [g.exist_since_iter_, g.xyz_gradient_accum_, g.denom_, g.max_radii2D_]:
            assert t.shape[0] == P + n
        assert bool((g.exist_since_iter_[P:] == 17).all()) and bool((g.exist_since_iter_[:P] == 0).all())
        a0, d0, gt = m0["alpha"].reshape(-1), m0["depth"].reshape(-1), m0["gt"].reshape(-1)
        with np.errstate(invalid="ignore"):
            fired = (d0 > gt) & (np.abs(gt - d0) > T)
        assert np.all((a0[pix] < f32(0.5)) | fired[pix])
        m1 = _maps_of(ts, kf, gt_depth)
        x0, y0, x1, y1 = rect
        before, after = float(m0["alpha"][y0:y1, x0:x1].mean()), float(m1["alpha"][y0:y1, x0:x1].mean())
        print(f"measured: mean alpha over the rectangle before {before} after {after}; seeds {n}")
        assert after > before
        want2 = reference_select(m1, _ts_options(ts))
        n2 = ts.seedFromDepth(kf, gt_image, gt_depth, 18, want_pixels=True)
        assert n2 == want2[1][0] and g.last_seed_counts_ == want2[1]
        if n2:
            assert np.array_equal(g.last_seed_pixels_.cpu().numpy(), want2[0])
        print(f"measured: first call {n} rows, second call {n2} rows")
        # ---- a seed rendered alone lands on its pixel
        from photo_slam_amd.gaussian_model import GaussianModel
        for j in (0, n // 2, n - 1):
            one = GaussianModel(3, dev)
            for name in g._PARAM_NAMES:
                setattr(one, name, getattr(g, name).detach()[P + j:P + j + 1].clone().requires_grad_(True))
            one.active_sh_degree_ = 3
            _, ts1 = python_trainer(cl, dev)
            ts1.gaussians_ = one
            _, _, alpha1 = ts1.render_view(kf, with_depth=True)
            assert int(alpha1.reshape(-1).argmax()) == int(pix[j]), (j, int(alpha1.reshape(-1).argmax()), int(pix[j]))
        return n, n2
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_empty_and_caps(lib_path, dev):
    """an empty model is initialised from a frame; seed_max_new_ and mcmc_cap_max_ are respected to the row; a process group is refused"""
    import pytest
    gr, rp = _host_modules()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, kf, gt_image, gt_depth, inside, rect = host_frame(dev)
        W, H = kf.image_width_, kf.image_height_
        m = dict(W=W, H=H, gt=gt_depth.cpu().numpy())
        g, ts = python_trainer(None, dev, seed_stride_=2)
        want_pix, want_counts, _ = reference_select(m, _ts_options(ts), maps=False)
        n = ts.seedFromDepth(kf, gt_image, gt_depth, 3, want_pixels=True)
        assert n == want_counts[0] == want_counts[1] > 0 and g.xyz_.shape[0] == n
        assert np.array_equal(g.last_seed_pixels_.cpu().numpy(), want_pix)
        assert all(bool(torch.isfinite(t).all()) for t in g.params()) and bool((g.exist_since_iter_ == 3).all())
        g.active_sh_degree_ = 3
        _, _, alpha = ts.render_view(kf, with_depth=True)
        assert float(alpha.mean()) > 0.1
        # ---- the caps
        for attrs, want in ((dict(seed_max_new_=37), 37), (dict(seed_max_new_=0), 0), (dict(mcmc_=True, mcmc_cap_max_=11), 11),
                            (dict(mcmc_=True, mcmc_cap_max_=0), 0), (dict(mcmc_=True, mcmc_cap_max_=-5), 0)):
            g, ts = python_trainer(cl, dev)
            g.prunePoints(inside)
            P = int(g.xyz_.shape[0])
            if "mcmc_cap_max_" in attrs:
                attrs = dict(attrs, mcmc_cap_max_=P + attrs["mcmc_cap_max_"])
            for k, v in attrs.items():
                setattr(ts, k, v)
            n = ts.seedFromDepth(kf, gt_image, gt_depth, 5, want_pixels=True)
            assert n == want and g.xyz_.shape[0] == P + want, (attrs, n, want)
            if want:   # thinned evenly, not truncated
                full = reference_select(_maps_of_before(ts, kf, gt_depth, g, P), _ts_options(ts))[0]
                ranks, _ = thinning(len(full), want)
                assert np.array_equal(g.last_seed_pixels_.cpu().numpy(), full[ranks])
        g, ts = python_trainer(cl, dev)
        ts.world_size_ = 2
        with pytest.raises(RuntimeError, match="seedFromDepth is not supported with a process group"):
            ts.seedFromDepth(kf, gt_image, gt_depth, 5)
    finally:
        rp._LIB_OVERRIDE = prev


def _maps_of_before(ts, kf, gt_depth, g, P):
    """the maps of the model's first P rows (what the seeding call rendered)"""
    from photo_slam_amd.gaussian_model import GaussianModel
    old = GaussianModel(3, g.xyz_.device)
    for name in g._PARAM_NAMES:
        setattr(old, name, getattr(g, name).detach()[:P].clone().requires_grad_(True))
    old.active_sh_degree_ = g.active_sh_degree_
    keep, ts.gaussians_ = ts.gaussians_, old
    try:
        return _maps_of(ts, kf, gt_depth)
    finally:
        ts.gaussians_ = keep


def check_host_train_step_after_seeding(lib_path, dev, steps_before=2):
    """fused optimizer, lazy SH rows: the train step after seedFromDepth equals the same step on a model that was given the same rows
    through _append_rows (increasePcd's path) -- bit for bit on the emulator build; on the device, where the backward blend adds
    with float atomics and two runs of one program differ in the last bits, to the bars tests/test_cpp_host.py uses"""
    gr, rp = _host_modules()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, kf, gt_image, gt_depth, inside, rect = host_frame(dev)
        mask = torch.ones_like(gt_image)
        models = []
        for _ in range(2):
            g, ts = python_trainer(cl, dev)
            g.prunePoints(inside)
            for _ in range(steps_before):
                ts.trainForOneIteration(kf, gt_image, mask, sync_loss=False)
            assert g.optimizer_.is_lazy(g._features), "the SH rows are not stepped lazily: the test would not cover that state"
            models.append((g, ts))
        (ga, tsa), (gb, tsb) = models
        P = int(ga.xyz_.shape[0])
        if dev.type == "cpu":
            for a, b in zip(ga.params_raw(), gb.params_raw()):
                assert torch.equal(a.detach(), b.detach())
        tsa.seed_max_new_ = 400
        n = tsa.seedFromDepth(kf, gt_image, gt_depth, 9)
        assert n == 400
        rows = {name: getattr(ga, name).detach()[P:].clone() for name in ga._PARAM_NAMES}
        gb._append_rows(rows, 9)
        for g, ts in models:
            ts.trainForOneIteration(kf, gt_image, mask, sync_loss=False)
            g.sync_features()
        worst = 0.0
        for a, b in zip(ga.params(), gb.params()):
            assert a.shape == b.shape and a.shape[0] == P + n
            worst = max(worst, float((a.detach() - b.detach()).abs().max()))
            if dev.type == "cpu":
                assert torch.equal(a.detach(), b.detach())
            else:
                assert torch.allclose(a.detach(), b.detach(), rtol=1e-4, atol=1e-6)
        for pa, pb in zip(ga.params_raw(), gb.params_raw()):
            for key in ("exp_avg", "exp_avg_sq"):
                x, y = ga.optimizer_.state[id(pa)][key], gb.optimizer_.state[id(pb)][key]
                assert torch.equal(x, y) if dev.type == "cpu" else torch.allclose(x, y, rtol=1e-4, atol=1e-6)
        assert torch.equal(ga.exist_since_iter_, gb.exist_since_iter_)
        assert bool((ga.xyz_.detach()[P:] != rows["xyz_"]).any()), "the step after seeding did not move a seed"
        print("measured: largest parameter difference after the step, seedFromDepth against _append_rows:", worst)
    finally:
        rp._LIB_OVERRIDE = prev


def _cpp_keyframe(cam, dev):
    """the Python keyframe with the tan(FoV / 2) the C++ host forms from the field of view it is handed (tests/pose_grad_cases.py:
    _cam_args): float(2 atan(t)) halved and passed through the C library's tanf, as std::tan(float) is"""
    import ctypes.util
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.tanf.restype, libm.tanf.argtypes = C.c_float, [C.c_float]
    kf = GaussianKeyframe.from_camera(cam, dev)
    kf.tanfovx_ = float(libm.tanf(C.c_float(float(f32(2 * math.atan(cam.tanfovx)) * f32(0.5)))))
    kf.tanfovy_ = float(libm.tanf(C.c_float(float(f32(2 * math.atan(cam.tanfovy)) * f32(0.5)))))
    return kf


def check_host_cpp(ops, lib_path, dev):
    """the C++ host (GaussianModel::seedFromDepth, TrainStep::seedFromDepth and its seed_* options through ops_register.cpp) against the
    Python host on the pruned scene: the same count, the same pixels, identical bits in every parameter, moment and statistic and in
    exist_since_iter_; the caps; the train step after a seeding that left lazily stepped SH rows behind against the same step after
    appendRows; an empty model in both of its forms (no tensors, tensors of 0 rows); a process group is refused"""
    import pytest
    import pose_grad_cases as pg
    gr, rp = _host_modules()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, kf, gt_image, gt_depth, inside, rect = host_frame(dev)
        kf = _cpp_keyframe(cl.cameras[0], dev)
        g, ts = python_trainer(cl, dev)
        g.prunePoints(inside)
        P = int(g.xyz_.shape[0])
        n_py = ts.seedFromDepth(kf, gt_image, gt_depth, 17, want_pixels=True)
        pix_py = g.last_seed_pixels_.cpu()
        g2, ts2 = python_trainer(cl, dev, mcmc_=True)
        g2.prunePoints(inside)
        ts2.mcmc_cap_max_ = P + 23
        assert ts2.seedFromDepth(kf, gt_image, gt_depth, 17, want_pixels=True) == 23
    finally:
        rp._LIB_OVERRIDE = prev
    cam = cl.cameras[0]
    args = pg._cam_args(cam, dev)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        ops.trainer_prune_points(h, inside)
        n_cpp = ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 17)
        assert n_cpp == n_py > 0, (n_cpp, n_py)
        assert torch.equal(ops.trainer_last_seed_pixels(h).cpu(), pix_py)
        assert ops.trainer_last_seed_counts(h) == g.last_seed_counts_
        for a, b in zip(ops.trainer_params(h), g.params()):
            assert a.shape == b.shape and torch.equal(a.detach(), b.detach()), "seedFromDepth differs between the hosts"
        assert torch.equal(ops.trainer_exist_since_iter(h), g.exist_since_iter_)
        for a, b in zip(ops.trainer_stats(h), (g.xyz_gradient_accum_, g.denom_, g.max_radii2D_)):
            assert a.shape == b.shape and torch.equal(a, b) and bool((a == 0).all())
        moments_py = [g.optimizer_.moments(p)[k] for k in (0, 1) for p in g.params_raw()]
        for a, b in zip(ops.trainer_moments(h), moments_py):
            assert a.shape == b.shape and torch.equal(a, b) and bool((a[P:] == 0).all())
    finally:
        ops.trainer_destroy(h)
    # ---- the train step after seeding, with lazily stepped SH rows left behind by an in-place append: two C++ trainers take the same two
    # steps (the arena of the prune has room for 400 rows more, the SH rows of the Gaussians the view culls are steps behind), one is
    # seeded, the other is handed the same rows through appendRows, both take one more step
    mask = torch.ones_like(gt_image)
    hs = [pg.cpp_trainer(ops, cl, dev, deg=3) for _ in range(2)]
    try:
        for h in hs:
            ops.trainer_prune_points(h, inside)
            for _ in range(2):
                ops.trainer_render_and_backward(h, *args, gt_image, mask)
                ops.trainer_finish(h)
        ha, hb = hs
        before = ops.trainer_features_row_step(ha)
        assert before.numel() == P and bool((before < before.max()).any()), "no SH row is behind: the test would not cover the lazy state"
        ptrs = [t.data_ptr() for t in ops.trainer_state(ha)[:15]]
        ops.trainer_set_options(ha, {"seed_max_new": 400.0})
        assert ops.trainer_seed_from_depth(ha, *args, gt_image, gt_depth, 9) == 400
        after = ops.trainer_features_row_step(ha)
        assert [t.data_ptr() for t in ops.trainer_state(ha)[:15]] == ptrs, "the append was not in place"
        assert after.numel() == P + 400 and torch.equal(after[:P], before), "seeding did not keep the lazy state of the SH rows"
        assert bool((after[P:] == after.max()).all()), "a new row does not join up to date"
        rows = [t.detach()[P:].clone() for t in ops.trainer_state(ha)[:5]]   # (the leaves as they are: reading them flushes nothing)
        ops.trainer_append_rows(hb, rows, 9)
        assert torch.equal(ops.trainer_features_row_step(hb), after)
        for h in hs:
            ops.trainer_render_and_backward(h, *args, gt_image, mask)
            ops.trainer_finish(h)
        worst = 0.0
        both = [ops.trainer_params(h) + ops.trainer_moments(h) for h in hs]   # (both calls bring every SH row up to date)
        for a, b in zip(*both):
            assert a.shape == b.shape and a.shape[0] == P + 400
            worst = max(worst, float((a.detach() - b.detach()).abs().max()))
            if dev.type == "cpu":
                assert torch.equal(a.detach(), b.detach())
            else:   # (the backward blend adds with float atomics there: the bars of tests/test_cpp_host.py)
                assert torch.allclose(a.detach(), b.detach(), rtol=1e-4, atol=1e-6)
        assert torch.equal(ops.trainer_exist_since_iter(ha), ops.trainer_exist_since_iter(hb))
        assert bool((ops.trainer_params(ha)[0][P:] != rows[0]).any()), "the step after seeding did not move a seed"
        print("measured: C++ host, largest difference after the step, seedFromDepth against appendRows:", worst)
    finally:
        for h in hs:
            ops.trainer_destroy(h)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:   # the caps, to the row
        ops.trainer_prune_points(h, inside)
        ops.trainer_set_options(h, {"seed_max_new": 37.0})
        assert ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 5) == 37
        ops.trainer_set_options(h, {"mcmc": 1.0, "mcmc_cap_max": float(P + 37 + 23)})
        assert ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 5) == 23
        assert ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 5) == 0
        assert ops.trainer_params(h)[0].shape[0] == P + 60
        ops.trainer_set_factored_exchange(h, True)
        with pytest.raises(RuntimeError, match="seedFromDepth is not supported with a process group"):
            ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 5)
    finally:
        ops.trainer_destroy(h)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:   # an empty model: every row pruned, then initialised from the frame (no render: alpha and depth NULL)
        ops.trainer_prune_points(h, torch.ones(HOST_P, dtype=torch.bool, device=dev))
        assert ops.trainer_params(h)[0].shape[0] == 0
        ops.trainer_set_options(h, {"seed_stride": 2.0})
        m = dict(W=cam.W, H=cam.H, gt=gt_depth.cpu().numpy())
        o = dict(DEFAULTS, min_depth=0.1, max_depth=100.0, stride=2, depth_error_median_factor=50.0)
        want_pix, want_counts, _ = reference_select(m, o, maps=False)
        assert ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 2) == want_counts[0] > 0
        assert np.array_equal(ops.trainer_last_seed_pixels(h).cpu().numpy(), want_pix)
        zero_rows = [p.detach().clone() for p in ops.trainer_params(h)]
    finally:
        ops.trainer_destroy(h)
    h = ops.trainer_create_empty(3, torch.zeros(3, device=dev))
    try:   # ... and a model that has no tensors at all: the same rows
        ops.trainer_set_options(h, {"seed_stride": 2.0, "depth_min": 0.1, "depth_max": 100.0})
        assert ops.trainer_seed_from_depth(h, *args, gt_image, gt_depth, 2) == want_counts[0]
        assert np.array_equal(ops.trainer_last_seed_pixels(h).cpu().numpy(), want_pix)
        for a, b in zip(ops.trainer_params(h), zero_rows):
            assert a.shape == b.shape and torch.equal(a.detach(), b)
        assert bool((ops.trainer_exist_since_iter(h) == 2).all()) and all(t.shape[0] == want_counts[0] for t in ops.trainer_stats(h))
    finally:
        ops.trainer_destroy(h)

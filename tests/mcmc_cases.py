"""Shared checks of the 3DGS-MCMC kernels (gsr_mcmc_relocate, gsr_mcmc_add_noise; include/gsr.h) and of the hosts' relocateDead /
addNew / addPositionNoise, run by test_mcmc.py on the emulator build and by test_gpu_mcmc.py on the MI355X.

Every reference here is float64 numpy written from the definitions in include/gsr.h.  The sampling is checked EXACTLY: given the
weights the kernel emitted (out_weights, themselves held to 4 units of round(sigmoid64 * 2^24)), the source of every draw is
searchsorted(cumsum(w), t, 'right') -- integers, no tolerance.  The new values (o', scale', the stored logit and log-scale) and
the noise step carry the bars BAR_VALUES and BAR_NOISE; how they were set is written in the docstrings of the two test files."""
import ctypes as C

import numpy as np
import torch

from photo_slam_amd import capi

MIN_OPACITY = 0.005
# one workgroup of 256, its wave boundaries, several workgroups, and the first size past one chunk (1024 block totals of 256 rows)
# of the spine scan
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 33000]
PAST_ONE_CHUNK = 1024 * 256 + 300

# bars: the next power of ten above ten times the larger of the emulator's and the MI355X's largest error (test_mcmc.py,
# test_gpu_mcmc.py carry the measurements): 1.7e-5 and 8.1e-5 on both builds.  The alpha check measured exactly 0 on both, which
# sets no bar: it is ten times one float32 rounding of the alpha map's value (2^-24 = 6e-8), to the next power of ten.
BAR_VALUES = 1e-3
BAR_NOISE = 1e-3
BAR_ALPHA = 1e-6

NAMES = ("xyz", "features", "opacity", "scaling", "rotation")


def sigmoid64(x):
    with np.errstate(over="ignore"):   # (exp(1e4) = inf gives exactly 0, as wanted)
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def make_inputs(P, room=0, M=4, seed=0, dead_fraction=0.05, logits=None):
    """Normal(0, 2) logits with about 5 % of the rows forced dead (logit -8: o = 3.4e-4); xyz[:, 0] = the row number, so that a copied
    row names its source; moments, statistics and exist_since_iter hold recognisable non-zero values.  `room` rows follow the P
    live ones in every array (growth), filled with a sentinel."""
    rng = np.random.default_rng(seed)
    n = P + room
    f32 = np.float32
    d = {}
    d["xyz"] = rng.normal(size=(n, 3)).astype(f32)
    d["xyz"][:, 0] = np.arange(n, dtype=f32)
    d["features"] = rng.normal(size=(n, M, 3)).astype(f32)
    lg = rng.normal(0.0, 2.0, size=(n, 1)).astype(f32)
    if dead_fraction > 0:
        lg[rng.random(n) < dead_fraction] = -8.0
    if logits is not None:
        lg[:P, 0] = np.asarray(logits, f32)
    d["opacity"] = lg
    d["scaling"] = rng.normal(-1.0, 0.7, size=(n, 3)).astype(f32)
    d["rotation"] = rng.normal(size=(n, 4)).astype(f32)
    for name in NAMES:
        d["m1_" + name] = rng.normal(size=d[name].shape).astype(f32)
        d["m2_" + name] = rng.random(size=d[name].shape).astype(f32) + f32(0.5)
    d["exist"] = rng.integers(1, 1000, size=n).astype(np.int32)
    for k in range(3):
        d[f"stat{k}"] = rng.random(n).astype(f32) + f32(1.0)
    if room:
        for k, v in d.items():
            v[P:] = 777 if v.dtype == np.int32 else f32(-123.5)
    return d


def relocate(lib_path, dev, d, P, draws, n_add=0, min_opacity=MIN_OPACITY, moments=True, extras=True, want_weights=True,
             n_draws=None):
    """gsr_mcmc_relocate on copies of d's arrays; returns (status, arrays after, counts, weights)."""
    lib = capi.load(lib_path)
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in d.items()}
    draws_t = torch.from_numpy(np.asarray(draws, np.float32).copy()).to(dev)
    n_draws = int(draws_t.numel()) if n_draws is None else n_draws
    a = capi.McmcRelocateArgs()
    a.P, a.n_add, a.n_draws, a.min_opacity = P, n_add, n_draws, min_opacity
    a.features_row_floats = int(d["features"].shape[1] * d["features"].shape[2])
    for i, name in enumerate(NAMES):
        a.param[i] = t[name].data_ptr()
        if moments:
            a.exp_avg[i], a.exp_avg_sq[i] = t["m1_" + name].data_ptr(), t["m2_" + name].data_ptr()
    a.draws = draws_t.data_ptr() if draws_t.numel() else None
    if extras:
        a.exist_since_iter = t["exist"].data_ptr()
        for k in range(3):
            a.stats[k] = t[f"stat{k}"].data_ptr()
    weights = torch.full((max(P, 1),), -1, dtype=torch.int32, device=dev) if want_weights else None
    if weights is not None:
        a.out_weights = weights.data_ptr()
    scratch = torch.empty(int(lib.gsr_mcmc_scratch_bytes(P, n_draws)) + 256, dtype=torch.uint8, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream if dev.type != "cpu" else None
    st = lib.gsr_mcmc_relocate(C.byref(a), scratch.data_ptr(), counts.data_ptr(), stream)
    if dev.type != "cpu":
        torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    w = weights.cpu().numpy().view(np.uint32)[:P].astype(np.uint64) if weights is not None else None
    return st, out, counts.cpu().numpy(), w


def binom_D(on, N):
    """D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1), float64"""
    from math import comb
    D = 0.0
    for i in range(1, N + 1):
        for k in range(i):
            D += comb(i - 1, k) * (-1.0) ** k * on ** (k + 1) / np.sqrt(k + 1.0)
    return D


def new_values(logit, scaling, n, min_opacity=MIN_OPACITY):
    """(o', scale' [3], stored logit, stored log-scale [3]) of a source with N_s = n, float64"""
    N = min(int(n), 51)
    o = float(sigmoid64(np.float32(logit)))
    on = 1.0 - (1.0 - o) ** (1.0 / N)
    on = min(max(on, float(np.float32(min_opacity))), 1.0 - 2.0 ** -24)
    D = binom_D(on, N)
    sc = np.exp(np.asarray(scaling, np.float64)) * o / D
    return on, sc, np.log(on / (1.0 - on)), np.log(sc)


def expected_sources(w, draws, n_dest):
    """the exact sampling: t = min(uint64(float64(u) * float64(total)), total - 1); source = searchsorted(C, t, 'right')"""
    Cw = np.cumsum(w.astype(np.uint64), dtype=np.uint64)
    total = int(Cw[-1])
    u = np.asarray(draws, np.float32)[:n_dest].astype(np.float64)
    t = np.minimum((u * np.float64(total)).astype(np.uint64), np.uint64(total - 1))
    return np.searchsorted(Cw, t, side="right").astype(np.int64)


def check_relocate(lib_path, dev, P, n_add=0, draws=None, n_draws=None, seed=0, M=4, logits=None, dead_fraction=0.05,
                   moments=True, extras=True, min_opacity=MIN_OPACITY, d=None):
    """one call against the definition.  Returns (largest relative error of the new values, counts, outputs)."""
    d = make_inputs(P, room=n_add, M=M, seed=seed, dead_fraction=dead_fraction, logits=logits) if d is None else d
    rng = np.random.default_rng(seed + 1000)
    if draws is None:
        draws = rng.random(max(P, n_add)).astype(np.float32)
    draws = np.asarray(draws, np.float32)
    st, out, counts, w = relocate(lib_path, dev, d, P, draws, n_add=n_add, min_opacity=min_opacity, moments=moments, extras=extras,
                                  n_draws=n_draws)
    assert st == 0, st
    n_draws = len(draws) if n_draws is None else n_draws

    # ---- weights
    o64 = sigmoid64(d["opacity"][:P, 0])
    dead = o64 <= float(np.float32(min_opacity))
    want_w = np.rint(o64 * 2.0 ** 24)
    if n_add == 0:
        assert np.all(w[dead] == 0), "a dead row kept a weight while relocating"
        want_w[dead] = 0
    worst_w = float(np.abs(w.astype(np.float64) - want_w).max())
    print("measured: weights, largest difference from round(sigmoid64 * 2^24):", worst_w, "units")
    assert worst_w <= 4, worst_w

    # ---- destinations and their sources, exactly
    total = int(w.sum())
    dead_rows = np.flatnonzero(dead)
    if total == 0:
        dests = np.zeros(0, np.int64)
    elif n_add > 0:
        dests = P + np.arange(n_add)
    else:
        dests = dead_rows[:min(len(dead_rows), n_draws)]
    src = expected_sources(w, draws, len(dests)) if len(dests) else np.zeros(0, np.int64)
    got_src = np.rint(out["xyz"][dests, 0]).astype(np.int64)   # xyz[:, 0] of a copied row is its source's row number
    assert np.array_equal(got_src, src), (np.flatnonzero(got_src != src)[:5], got_src[:5], src[:5])
    n_of = 1 + np.bincount(src, minlength=P)
    sources = np.flatnonzero(n_of > 1)
    assert counts[0] == len(dead_rows) and counts[1] == len(dests), (counts, len(dead_rows), len(dests))
    assert counts[2] == len(sources) and counts[3] == (n_of.max() if len(sources) else 0), (counts, len(sources), n_of.max())
    assert np.all(counts[4:] == 0)

    # ---- the sources' rewrite against the definition
    worst = 0.0
    for s in sources:
        on, sc, lg, ls = new_values(d["opacity"][s, 0], d["scaling"][s], n_of[s], min_opacity)
        got_lg, got_ls = np.float64(out["opacity"][s, 0]), out["scaling"][s].astype(np.float64)
        errs = [abs(sigmoid64(got_lg) - on) / on, np.abs(np.exp(got_ls) - sc).max() / sc.max(),
                abs(got_lg - lg) / max(1.0, abs(lg)), (np.abs(got_ls - ls) / np.maximum(1.0, np.abs(ls))).max()]
        worst = max(worst, float(max(errs)))
    print("measured: new values (o', scale', stored logit and log-scale), largest relative error:", worst, "over", len(sources), "sources")
    assert worst <= BAR_VALUES, worst

    # ---- destinations: copies of the source's xyz / SH / rotation and of its NEW opacity and scale, bit for bit
    for name in NAMES:
        assert np.array_equal(out[name][dests].view(np.uint32), out[name][src].view(np.uint32)), name
    touched_param = {name: np.zeros(len(d[name]), bool) for name in NAMES}
    for name in NAMES:
        touched_param[name][dests] = True
    touched_param["opacity"][sources] = True
    touched_param["scaling"][sources] = True
    zeroed = np.zeros(len(d["xyz"]), bool)
    zeroed[dests] = True
    zeroed[sources] = True
    for name in NAMES:
        same = ~touched_param[name]
        assert np.array_equal(out[name][same].view(np.uint32), d[name][same].view(np.uint32)), f"{name}: a row that took no part changed"
        for m in ("m1_", "m2_"):
            if moments:
                assert np.all(out[m + name][zeroed].view(np.uint32) == 0), f"{m}{name}: not exactly zero at a source or a destination"
                assert np.array_equal(out[m + name][~zeroed].view(np.uint32), d[m + name][~zeroed].view(np.uint32)), m + name
            else:
                assert np.array_equal(out[m + name].view(np.uint32), d[m + name].view(np.uint32)), m + name
    is_dest = np.zeros(len(d["xyz"]), bool)
    is_dest[dests] = True
    if extras:
        assert np.array_equal(out["exist"][dests], d["exist"][src]) and np.array_equal(out["exist"][~is_dest], d["exist"][~is_dest])
        for k in range(3):
            assert np.all(out[f"stat{k}"][dests].view(np.uint32) == 0), "a destination's statistics are not zero"
            assert np.array_equal(out[f"stat{k}"][~is_dest].view(np.uint32), d[f"stat{k}"][~is_dest].view(np.uint32))
    else:
        assert np.array_equal(out["exist"], d["exist"]) and all(np.array_equal(out[f"stat{k}"], d[f"stat{k}"]) for k in range(3))
    return worst, counts, out


def check_edge_draws(lib_path, dev):
    """draws 0.0 and 1 - 2^-24, and draws landing exactly on prefix boundaries: 48 live rows of logit 0 have w = 2^23 each (sigmoid(0)
    is exactly 0.5), the total is 3 * 2^27 and u = j / 4 gives t = 3 j 2^25 = C of the (12 j)-th live row exactly -- the first s
    with C[s] > t is the live row AFTER it (and never one of the dead rows in between, whose C equals their predecessor's)"""
    P = 64
    logits = np.zeros(P, np.float32)
    logits[1::4] = -8.0    # 16 dead rows
    live = np.flatnonzero(logits == 0)
    draws = np.array([0.0, 1.0 - 2.0 ** -24, 0.25, 0.5, 0.75] + [0.125] * 11, np.float32)
    worst, counts, out = check_relocate(lib_path, dev, P, draws=draws, logits=logits, dead_fraction=0.0)
    dests = np.flatnonzero(logits == -8.0)
    got = np.rint(out["xyz"][dests[:5], 0]).astype(int)
    assert list(got) == [live[0], live[-1], live[12], live[24], live[36]], got
    return worst


def check_all_dead(lib_path, dev, P=300):
    """every row dead: no weight anywhere, nothing moves, counts = [P, 0, 0, 0]"""
    d = make_inputs(P, logits=np.full(P, -9.0, np.float32))
    st, out, counts, w = relocate(lib_path, dev, d, P, np.random.default_rng(0).random(P))
    assert st == 0 and list(counts) == [P, 0, 0, 0, 0, 0, 0, 0], counts
    assert np.all(w == 0)
    for k in d:
        assert np.array_equal(out[k].view(np.uint32), d[k].view(np.uint32)), k


def check_none_dead(lib_path, dev, P=300):
    d = make_inputs(P, dead_fraction=0.0, logits=np.random.default_rng(3).normal(1.0, 1.0, P))
    st, out, counts, w = relocate(lib_path, dev, d, P, np.random.default_rng(0).random(P))
    assert st == 0 and list(counts) == [0] * 8, counts
    for k in d:
        assert np.array_equal(out[k].view(np.uint32), d[k].view(np.uint32)), k


def check_fewer_draws_than_dead(lib_path, dev, P=1025):
    """n_draws < dead rows: the surplus dead rows are untouched bit for bit (check_relocate's 'took no part' comparison covers them)"""
    d = make_inputs(P, dead_fraction=0.2, seed=5)
    dead = int((sigmoid64(d["opacity"][:, 0]) <= MIN_OPACITY).sum())
    n = dead // 2
    worst, counts, _ = check_relocate(lib_path, dev, P, d=d, draws=np.random.default_rng(1).random(n).astype(np.float32))
    assert counts[0] == dead and counts[1] == n
    # ... and the same through n_draws alone, with a longer array behind it
    check_relocate(lib_path, dev, P, d=d, draws=np.random.default_rng(1).random(P).astype(np.float32), n_draws=n)
    return worst


def check_one_source_60_times(lib_path, dev):
    """60 dead rows all drawing row 7: N = 61, the formulas use 51"""
    P = 130
    logits = np.random.default_rng(2).normal(0.5, 1.0, P).astype(np.float32)
    logits[70:] = -8.0
    logits[7] = 3.0
    d = make_inputs(P, dead_fraction=0.0, logits=logits)
    w = np.rint(sigmoid64(logits) * 2.0 ** 24)
    w[70:] = 0
    Cw = np.cumsum(w)
    u = np.float32((Cw[6] + 0.5 * w[7]) / Cw[-1])
    worst, counts, out = check_relocate(lib_path, dev, P, d=d, draws=np.full(60, u, np.float32))
    assert counts[1] == 60 and counts[2] == 1 and counts[3] == 61, counts
    on, sc, lg, ls = new_values(logits[7], d["scaling"][7], 51)
    assert abs(np.float64(out["opacity"][7, 0]) - lg) <= BAR_VALUES * abs(lg)
    return worst


def check_growth(lib_path, dev, P, n_add, seed=0):
    """rows [P, P + n_add) are filled from draws over ALL rows (a dead source is allowed); rows < P that were not drawn are
    unchanged (check_relocate's comparison)"""
    return check_relocate(lib_path, dev, P, n_add=n_add, seed=seed, dead_fraction=0.1)[0]


def check_determinism(lib_path, dev, P=33000):
    d = make_inputs(P, room=1000, seed=9)
    draws = np.random.default_rng(4).random(P).astype(np.float32)
    for n_add in (0, 1000):
        a = relocate(lib_path, dev, d, P, draws, n_add=n_add)
        b = relocate(lib_path, dev, d, P, draws, n_add=n_add)
        for k in d:
            assert np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)), k
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    z = np.random.default_rng(5).normal(size=(P, 3)).astype(np.float32)
    x = noise(lib_path, dev, d, P, z, 0.3)
    y = noise(lib_path, dev, d, P, z, 0.3)
    assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))


def check_api_contract(lib_path, dev):
    lib = capi.load(lib_path)
    d = make_inputs(64)
    draws = np.random.default_rng(0).random(64).astype(np.float32)
    INVALID = -1
    assert lib.gsr_strerror(INVALID) is not None
    base = dict(P=64, draws=draws)
    st, _, _, _ = relocate(lib_path, dev, d, 64, draws)
    assert st == 0

    def status(**kw):
        lib_ = capi.load(lib_path)
        t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in d.items()}
        dr = torch.from_numpy(draws.copy()).to(dev)
        a = capi.McmcRelocateArgs()
        a.P, a.n_add, a.n_draws, a.min_opacity, a.features_row_floats = 64, 0, 64, MIN_OPACITY, 12
        for i, name in enumerate(NAMES):
            a.param[i], a.exp_avg[i], a.exp_avg_sq[i] = t[name].data_ptr(), t["m1_" + name].data_ptr(), t["m2_" + name].data_ptr()
        a.draws = dr.data_ptr()
        scratch = torch.empty(int(lib_.gsr_mcmc_scratch_bytes(64, 64)) + 256, dtype=torch.uint8, device=dev)
        counts = torch.full((8,), -1, dtype=torch.int32, device=dev)
        sp, cp = scratch.data_ptr(), counts.data_ptr()
        for k, v in kw.items():
            if k == "scratch":
                sp = v
            elif k == "counts":
                cp = v
            elif isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        st_ = lib_.gsr_mcmc_relocate(C.byref(a), sp, cp, None)
        return st_, counts.cpu().numpy()

    assert status()[0] == 0
    for kw in (dict(P=-1), dict(n_add=-1), dict(n_add=65), dict(draws=None), dict(scratch=None), dict(counts=None),
               dict(param=(2, None)), dict(param=(0, None)), dict(exp_avg=(3, None)), dict(exp_avg_sq=(0, None)),
               dict(min_opacity=0.0), dict(min_opacity=1.0), dict(min_opacity=-0.5), dict(min_opacity=float("nan")),
               dict(features_row_floats=0)):
        assert status(**kw)[0] == INVALID, kw
    assert lib.gsr_mcmc_relocate(None, None, None, None) == INVALID
    st, counts = status(P=0, scratch=None)
    assert st == 0 and list(counts) == [0] * 8, (st, counts)
    assert lib.gsr_mcmc_scratch_bytes(0, 0) > 0 and lib.gsr_mcmc_scratch_bytes(1000, 1000) > lib.gsr_mcmc_scratch_bytes(10, 10)
    assert lib.gsr_mcmc_scratch_bytes(-5, -5) == lib.gsr_mcmc_scratch_bytes(0, 0)
    # the noise call
    x = torch.zeros((4, 3), device=dev)
    q = torch.ones((4, 4), device=dev)
    assert lib.gsr_mcmc_add_noise(-1, x.data_ptr(), x.data_ptr(), x.data_ptr(), q.data_ptr(), x.data_ptr(), 1.0, None) == INVALID
    assert lib.gsr_mcmc_add_noise(0, None, None, None, None, None, 1.0, None) == 0
    for hole in range(5):
        p = [x.data_ptr(), x.data_ptr(), x.data_ptr(), q.data_ptr(), x.data_ptr()]
        p[hole] = None
        assert lib.gsr_mcmc_add_noise(4, *p, 1.0, None) == INVALID, hole


# ------------------------------------------------------------------------------------------------------------ the noise step
def noise(lib_path, dev, d, P, z, noise_scale):
    lib = capi.load(lib_path)
    t = {k: torch.from_numpy(d[k][:P].copy()).to(dev) for k in ("xyz", "opacity", "scaling", "rotation")}
    zt = torch.from_numpy(np.asarray(z, np.float32).copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream if dev.type != "cpu" else None
    st = lib.gsr_mcmc_add_noise(P, t["xyz"].data_ptr(), t["opacity"].data_ptr(), t["scaling"].data_ptr(), t["rotation"].data_ptr(),
                                zt.data_ptr(), float(noise_scale), stream)
    if dev.type != "cpu":
        torch.cuda.synchronize()
    return st, t["xyz"].cpu().numpy()


def noise_reference(d, P, z, noise_scale):
    """the displacement Sigma (z g noise_scale) in float64"""
    o = sigmoid64(d["opacity"][:P, 0])
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(100.0 * (o - 0.005)))
    q = d["rotation"][:P].astype(np.float64)
    q = q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), 1e-12)
    r, x, y, zq = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y),
                  2 * (x * y + r * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x),
                  2 * (x * zq - r * y), 2 * (y * zq + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s2 = np.exp(d["scaling"][:P].astype(np.float64)) ** 2
    Sigma = np.einsum("nij,nj,nkj->nik", R, s2, R)
    v = np.asarray(z, np.float64) * (g * np.float64(np.float32(noise_scale)))[:, None]
    return np.einsum("nij,nj->ni", Sigma, v), g


def noise_inputs(P, seed=0):
    """low opacities (where g is not negligible) mixed with ordinary ones, non-unit quaternions, anisotropic scales"""
    rng = np.random.default_rng(seed)
    d = make_inputs(P, seed=seed, dead_fraction=0.0)
    lg = rng.normal(-4.0, 2.0, P).astype(np.float32)
    d["opacity"][:P, 0] = lg
    d["rotation"][:P] *= rng.uniform(0.2, 5.0, size=(P, 1)).astype(np.float32)
    d["scaling"][:P] = rng.normal(-1.0, 1.0, size=(P, 3)).astype(np.float32)
    d["xyz"][:P, 0] = rng.normal(size=P).astype(np.float32)
    return d


def check_noise(lib_path, dev, P, noise_scale=0.5, seed=0):
    """xyz + Sigma (z g noise_scale) against float64.  The error is measured on the displacement, relative to the row's largest
    displacement component; one rounding of the fp32 sum xyz + displacement (2^-24 |xyz'|) is allowed beside it."""
    d = noise_inputs(P, seed)
    z = np.random.default_rng(seed + 50).normal(size=(P, 3)).astype(np.float32)
    st, got = noise(lib_path, dev, d, P, z, noise_scale)
    assert st == 0
    disp, g = noise_reference(d, P, z, noise_scale)
    want = d["xyz"][:P].astype(np.float64) + disp
    assert np.all(np.isfinite(got))
    scale = np.abs(disp).max(1, keepdims=True)
    excess = np.maximum(np.abs(got.astype(np.float64) - want) - 2.0 ** -24 * np.abs(want), 0.0)
    moving = scale[:, 0] > 1e-30
    worst = float((excess[moving] / scale[moving]).max()) if moving.any() else 0.0
    print("measured: noise step, largest error of the displacement relative to the row's largest component:", worst)
    assert worst <= BAR_NOISE, worst
    assert np.array_equal(got[~moving].view(np.uint32), d["xyz"][:P][~moving].view(np.uint32))
    return worst


def check_noise_corners(lib_path, dev):
    P = 8
    d = noise_inputs(P, seed=3)
    # o = 0.9, o -> 1 (logit 20, 40, 1e4): exactly no motion, finite; o = 0.005: g = 0.5
    lg = np.array([np.log(0.9 / 0.1), 20.0, 40.0, 1e4, np.log(0.005 / 0.995), -3.0, -30.0, -1e4], np.float32)
    d["opacity"][:P, 0] = lg
    z = np.random.default_rng(1).normal(size=(P, 3)).astype(np.float32)
    st, got = noise(lib_path, dev, d, P, z, 2.0)
    assert st == 0 and np.all(np.isfinite(got))
    assert np.array_equal(got[:4].view(np.uint32), d["xyz"][:4].view(np.uint32)), "an opaque Gaussian moved"
    disp, g = noise_reference(d, P, z, 2.0)
    assert abs(g[4] - 0.5) < 1e-4    # (logit of 0.005 in fp32: o = 0.005 to 1e-9, times the slope 25 of g there)
    moved = got[4:].astype(np.float64) - d["xyz"][4:P]
    assert np.allclose(moved, disp[4:], rtol=1e-3, atol=1e-7), (moved, disp[4:])
    assert np.all(np.abs(moved[0]) > 0)
    # noise_scale = 0: bit-identical
    st, same = noise(lib_path, dev, d, P, z, 0.0)
    assert st == 0 and np.array_equal(same.view(np.uint32), d["xyz"][:P].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ the hosts
def _host_modules():
    import geom_reg_cases as gr
    from photo_slam_amd import rasterize_points as rp
    return gr, rp


def alpha_at_centre(lib_path, dev, o, k):
    """What the formula is for: one Gaussian of opacity o whose mean projects onto the centre of pixel (48, 32) of a 96 x 64 view, plus k
    dead rows elsewhere.  Returns (out_alpha at that pixel before relocateDead, after it, the counts)."""
    import copy
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_model import GaussianModel
    cl = gr.cloud(1 + k)
    cam = cl.cameras[0]
    px, py = 48, 32
    right, up, fwd = (cam.viewmatrix[:3, j].astype(np.float64) for j in range(3))

    def pixel(p):   # the rasterizer's mean2D = ((ndc + 1) S - 1) / 2, float64
        h = np.append(p, 1.0) @ cam.projmatrix.astype(np.float64)
        return np.array([((h[0] / h[3] + 1.0) * cam.W - 1.0) * 0.5, ((h[1] / h[3] + 1.0) * cam.H - 1.0) * 0.5])
    base = cam.campos.astype(np.float64) + 2.5 * fwd
    J = np.stack([pixel(base + right) - pixel(base), pixel(base + up) - pixel(base)], 1)   # (affine at a fixed depth)
    uv = np.linalg.solve(J, np.array([px, py], np.float64) - pixel(base))
    centre = base + uv[0] * right + uv[1] * up
    assert np.abs(pixel(centre) - [px, py]).max() < 1e-9
    cl.xyz[:] = (base + 0.8 * right).astype(np.float32)           # the dead rows: somewhere else in the view
    cl.xyz[0] = centre.astype(np.float32)
    cl.scaling[:] = np.float32(np.log(0.15))                       # (about 5 px at 2.5 m and f = 80)
    cl.rotation[:] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    cl.opacity[:] = np.float32(-9.0)
    cl.opacity[0] = np.float32(np.log(o / (1.0 - o)))
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        def alpha(c):
            a = gr.model_inputs(c, cam, dev, raw=gr.ALL_RAW)
            out = torch.zeros((cam.H, cam.W), device=dev)
            rp.RasterizeGaussiansCUDA(**dict(a, degree=3), raw_params=gr.ALL_RAW | capi.FORWARD_ONLY, out_alpha=out)
            return float(out[py, px])
        before = alpha(cl)
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        counts = g.relocateDead(MIN_OPACITY, generator=torch.Generator(device=dev).manual_seed(1)).cpu().numpy()
        after_cl = copy.deepcopy(cl)
        after_cl.xyz, after_cl.opacity = g.xyz_.detach().cpu().numpy(), g.opacity_.detach().cpu().numpy()
        after_cl.scaling, after_cl.rotation = g.scaling_.detach().cpu().numpy(), g.rotation_.detach().cpu().numpy()
        return before, alpha(after_cl), counts
    finally:
        rp._LIB_OVERRIDE = prev


def check_alpha_is_kept(lib_path, dev, o, k):
    before, after, counts = alpha_at_centre(lib_path, dev, o, k)
    assert list(counts[:4]) == [k, k, 1, k + 1], counts
    err = abs(after - before) / before
    print(f"measured: out_alpha at the centre, o = {o}, {k} dead rows: before {before!r} after {after!r} relative difference {err}")
    assert abs(before - o) < 1e-5 * o, (before, o)
    assert err <= BAR_ALPHA, (before, after)
    return err


def mcmc_cloud(P=300, dead=30):
    """the 96 x 64 scene of geom_reg_cases with `dead` rows started dead"""
    gr, _ = _host_modules()
    cl = gr.cloud(P, seed=4, scale_k=0.05)
    cl.opacity[np.random.default_rng(5).choice(P, dead, replace=False)] = np.float32(-8.0)
    return cl


HOST_INTERVAL = 10


def python_mcmc_trainer(cl, dev, cap, mcmc=True, **attrs):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    opt.lambda_dssim_ = 0.0
    opt.densify_from_iter_, opt.densification_interval_, opt.opacity_reset_interval_ = 0, HOST_INTERVAL, 20
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7, densify=True)
    ts.mcmc_, ts.mcmc_cap_max_ = mcmc, cap
    for k, v in attrs.items():
        setattr(ts, k, v)
    return g, ts


def _dead_count(g, min_opacity=MIN_OPACITY):
    return int((torch.sigmoid(g.opacity_.detach()) <= np.float32(min_opacity)).sum())


def _pointers(g):
    p = [t.data_ptr() for t in g.params_raw()]
    for t in g.params_raw():
        st = g.optimizer_.state.get(id(t))
        p += [st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()] if st else [0, 0]
    return p + [g.exist_since_iter_.data_ptr(), g.xyz_gradient_accum_.data_ptr(), g.denom_.data_ptr(), g.max_radii2D_.data_ptr()]


def check_host_training(lib_path, dev, steps=60):
    """mcmc_ on, cap = 1.2 x the initial count, densification interval 10.  The first 30 steps are the three events the issue's run has
    (300 -> 315 -> 330 -> 346: 1.05^3 < 1.2, the cap is not reached yet); the run goes on to 60 so that the count reaches exactly the
    cap at the fourth event and two relocation-only events follow.  After every event no row is dead; on the relocation-only
    events no tensor, moment, statistic or exist_since_iter_ is re-seated, with rows killed by hand just before so that they have work
    to do; the opacity is never reset (interval 20 here)."""
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = mcmc_cloud()
    P0 = cl.xyz.shape[0]
    cap = (P0 * 12) // 10
    cam = cl.cameras[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        gt = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(0)).to(dev)
        mask = torch.ones_like(gt)
        g, ts = python_mcmc_trainer(cl, dev, cap)

        def refuse(*a, **k):
            raise AssertionError("densifyAndPrune / resetOpacity with mcmc_ on")
        g.densifyAndPrune = g.resetOpacity = refuse
        want, sizes, reseated = P0, [], []
        for it in range(1, steps + 1):
            event = it % HOST_INTERVAL == 0
            if event and want == cap:   # a relocation-only event: give it work
                with torch.no_grad():
                    g.opacity_[3:13] = -8.0
                before_ptrs = _pointers(g)
            xyz_before = g.xyz_.detach().clone()
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
            if event:
                relocation_only = want == cap
                want = min(cap, (105 * want) // 100)
                assert g.xyz_.shape[0] == want, (it, g.xyz_.shape[0], want)
                for t in g.params_raw() + [g.exist_since_iter_, g.xyz_gradient_accum_, g.denom_, g.max_radii2D_]:
                    assert t.shape[0] == want
                assert _dead_count(g) == 0, (it, _dead_count(g))
                c = ts.last_mcmc_counts_.cpu().numpy()
                if it == HOST_INTERVAL:
                    assert c[0] >= 30 and c[1] == c[0], c
                if relocation_only:
                    assert c[0] >= 10 and c[1] == c[0], c
                    assert _pointers(g) == before_ptrs, "a relocation-only event re-seated a tensor"
                    reseated.append(it)
                sizes.append(want)
            else:
                assert g.xyz_.shape[0] == want
        assert sizes[:3] == [315, 330, 346] and sizes[3:] == [cap] * (len(sizes) - 3), sizes
        assert len(reseated) >= 2
        assert all(bool(torch.isfinite(t).all()) for t in g.params())
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return sizes
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_noise_runs_every_step(lib_path, dev):
    """with mcmc_ on every step moves the positions of low-opacity Gaussians the view does not see (Adam leaves them alone: the noise
    is the only thing that can move them), by exactly addPositionNoise's step from the trainer's generator"""
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = mcmc_cloud(dead=0)
    cam = cl.cameras[0]
    behind = cam.campos - 3.0 * cam.viewmatrix[:3, 2]
    cl.xyz[:20] = behind + np.random.default_rng(0).normal(size=(20, 3)).astype(np.float32) * 0.1
    cl.opacity[:20] = np.float32(-4.0)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        gt = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(0)).to(dev)
        mask = torch.ones_like(gt)
        moved = {}
        for on in (False, True):
            g, ts = python_mcmc_trainer(cl, dev, cl.xyz.shape[0], mcmc=on)
            x0 = g.xyz_.detach().clone()
            lr = None
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
            lr = g.optimizer_.param_groups[0]["lr"]
            moved[on] = (g.xyz_.detach() - x0)[:20].abs().max().item()
            if on:
                # the same draw, by hand, on the rows Adam did not touch
                gen = torch.Generator(device=dev).manual_seed(7)
                z = torch.empty((cl.xyz.shape[0], 3), device=dev).normal_(generator=gen)
                d = {k: getattr(cl, k) for k in ("xyz", "opacity", "scaling", "rotation")}
                disp, _ = noise_reference(d, cl.xyz.shape[0], z.cpu().numpy(), 5e5 * lr)
                got = (g.xyz_.detach() - x0)[:20].cpu().numpy().astype(np.float64)
                assert np.allclose(got, disp[:20], rtol=1e-3, atol=1e-7 * np.abs(disp[:20]).max()), (got[:2], disp[:2])
        assert moved[False] == 0.0 and moved[True] > 0.0, moved
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_off_is_off(lib_path, dev, steps=30):
    """mcmc_ False: over 30 steps with densification at interval 10 none of relocateDead / addNew / addPositionNoise is ever called,
    whatever the other mcmc_* attributes hold; densifyAndPrune and the opacity reset run as before.  On the emulator build, where a
    train step gives the same bits on every run, the two runs' parameters are compared bit for bit as well (on the device the
    backward blend adds its partial sums with float atomics: two runs of the SAME program differ in the last bits there, so
    that comparison would not test this feature)."""
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = mcmc_cloud()
    cam = cl.cameras[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        gt = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(0)).to(dev)
        mask = torch.ones_like(gt)
        runs = []
        for attrs in (dict(), dict(mcmc_cap_max_=5, mcmc_noise_lr_=1e9, mcmc_min_opacity_=0.5)):
            g, ts = python_mcmc_trainer(cl, dev, 0, mcmc=False, **attrs)
            if not attrs:
                for name in ("mcmc_", "mcmc_cap_max_"):
                    assert getattr(ts, name) in (False, 0)

            def refuse(*a, **k):
                raise AssertionError("an mcmc call with mcmc_ off")
            g.relocateDead = g.addNew = g.addPositionNoise = refuse
            resets = []
            reset = g.resetOpacity
            g.resetOpacity = lambda *a, **k: (resets.append(ts.iteration_), reset(*a, **k))[1]
            for _ in range(steps):
                ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
            g.sync_features()
            assert ts.last_densify_ is not None and ts.last_mcmc_counts_ is None and resets == [20], resets
            runs.append([p.detach().cpu().numpy() for p in g.params()])
        if dev.type == "cpu":
            for a, b in zip(*runs):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_model_calls(lib_path, dev):
    """GaussianModel.relocateDead / addNew / addPositionNoise directly: addNew on both sides of min(cap, 105 P / 100) and n_add = 0;
    rows < P that were not drawn are unchanged by addNew; relocateDead returns the device counts and re-seats nothing"""
    import copy
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    cl = mcmc_cloud()
    P = cl.xyz.shape[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        for cap, want in ((P + 1000, (105 * P) // 100), (P + 7, P + 7), (P, P), (P - 5, P)):
            g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
            g.trainingSetup(GaussianOptimizationParams())
            gen = torch.Generator(device=dev).manual_seed(3)
            before = [p.detach().clone() for p in g.params()]
            n = g.addNew(cap, generator=gen)
            assert n == want - P and g.xyz_.shape[0] == want, (cap, n, want)
            if n:
                src = g.xyz_.detach()[P:, None, :].eq(before[0][None, :, :]).all(2)
                assert bool(src.any(1).all()), "a new row is not a copy of an old one"
                drawn = src.any(0)
                for a, b in zip(before, g.params()):
                    assert torch.equal(a[~drawn], b.detach()[:P][~drawn]), "addNew changed a row that was not drawn"
                assert bool((g.opacity_.detach()[:P][drawn] != before[2][drawn]).all())
                for t in g.params_raw():
                    st = g.optimizer_.state[id(t)]
                    assert bool((st["exp_avg"][P:] == 0).all()) and bool((st["exp_avg_sq"][P:] == 0).all())
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        g.trainingSetup(GaussianOptimizationParams())
        leaves = [id(p) for p in g.params_raw()]
        ptrs = [p.data_ptr() for p in g.params_raw()]
        counts = g.relocateDead(generator=torch.Generator(device=dev).manual_seed(3))
        assert counts.device.type == dev.type and counts.dtype == torch.int32 and tuple(counts.shape) == (8,)
        assert counts[0].item() == 30 and counts[1].item() == 30 and _dead_count(g) == 0
        assert [id(p) for p in g.params_raw()] == leaves and [p.data_ptr() for p in g.params_raw()] == ptrs
        x0 = g.xyz_.detach().clone()
        g.addPositionNoise(0.0, generator=torch.Generator(device=dev).manual_seed(3))
        assert torch.equal(g.xyz_.detach(), x0)
        g.addPositionNoise(10.0, generator=torch.Generator(device=dev).manual_seed(3))
        assert not torch.equal(g.xyz_.detach(), x0) and bool(torch.isfinite(g.xyz_).all())
    finally:
        rp._LIB_OVERRIDE = prev


def check_process_group_is_refused(lib_path, dev):
    gr, rp = _host_modules()
    import pytest
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = mcmc_cloud()
    cam = cl.cameras[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = python_mcmc_trainer(cl, dev, 400)
        ts.world_size_ = 2
        gt = torch.zeros(3, cam.H, cam.W, device=dev)
        with pytest.raises(RuntimeError, match="mcmc_ is not supported with a process group"):
            ts.trainForOneIteration(GaussianKeyframe.from_camera(cam, dev), gt, torch.ones_like(gt))
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_cpp(ops, lib_path, dev, steps=22):
    """the C++ host (GaussianModel::relocateDead / addNew / addPositionNoise, TrainStep::mcmc_ ... through ops_register.cpp) against the
    Python host: the three calls alone from equal seeds give the same bits; 22 train steps with mcmc on (events at 10 and 20) give the
    same counts, the same sizes and -- to the bars tests/test_cpp_host.py uses for that comparison (rtol 1e-4, atol 1e-6) -- the same
    parameters; a process group is refused"""
    import copy
    import pose_grad_cases as pg
    gr, rp = _host_modules()
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = mcmc_cloud()
    P0 = cl.xyz.shape[0]
    cap = P0 + 20
    cam = cl.cameras[0]
    gt = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(0)).to(dev)
    mask = torch.ones_like(gt)
    options = {"densify": 1.0, "mcmc": 1.0, "mcmc_cap_max": float(cap), "densify_from_iter": 0.0, "densification_interval": float(HOST_INTERVAL),
               "opacity_reset_interval": 20.0}
    # ---- the three calls alone
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        c_cpp = ops.trainer_relocate_dead(h, MIN_OPACITY, 11).cpu()
        n_cpp = ops.trainer_add_new(h, cap, 12)
        ops.trainer_add_position_noise(h, 0.7, 13)
        alone_cpp = [p.detach().clone() for p in ops.trainer_params(h)]
        assert ops.trainer_last_mcmc_counts(h).numel() == 0
    finally:
        ops.trainer_destroy(h)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        gen = lambda s: torch.Generator(device=dev).manual_seed(s)
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        g.trainingSetup(GaussianOptimizationParams())
        c_py = g.relocateDead(MIN_OPACITY, generator=gen(11)).cpu()
        n_py = g.addNew(cap, generator=gen(12))
        g.addPositionNoise(0.7, generator=gen(13))
        assert torch.equal(c_cpp, c_py) and n_cpp == n_py == 15, (c_cpp, c_py, n_cpp, n_py)
        for a, b in zip(alone_cpp, g.params()):
            assert a.shape == b.shape and torch.equal(a, b.detach()), "relocateDead / addNew / addPositionNoise differ between the hosts"
    finally:
        rp._LIB_OVERRIDE = prev
    # ---- the train step
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        ops.trainer_set_options(h, options)
        sizes_cpp, counts_cpp = [], []
        for it in range(1, steps + 1):
            ops.trainer_render_and_backward(h, *pg._cam_args(cam, dev), gt, mask)
            before = [t.data_ptr() for t in ops.trainer_state(h)[:15]]
            ops.trainer_finish(h)
            sizes_cpp.append(int(ops.trainer_params(h)[0].shape[0]))
            if it % HOST_INTERVAL == 0:
                counts_cpp.append(ops.trainer_last_mcmc_counts(h).cpu().clone())
            if it == 20:   # (at the cap since the first event: relocation only)
                assert [t.data_ptr() for t in ops.trainer_state(h)[:15]] == before, "a relocation-only event re-seated a tensor"
        params_cpp = [p.detach().clone() for p in ops.trainer_params(h)]
    finally:
        ops.trainer_destroy(h)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        g, ts = python_mcmc_trainer(cl, dev, cap)
        g.active_sh_degree_ = 3
        sizes_py, counts_py = [], []
        for it in range(1, steps + 1):
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
            sizes_py.append(int(g.xyz_.shape[0]))
            if it % HOST_INTERVAL == 0:
                counts_py.append(ts.last_mcmc_counts_.cpu().clone())
        g.sync_features()
    finally:
        rp._LIB_OVERRIDE = prev
    assert sizes_cpp == sizes_py and sizes_py[9] == P0 + 15 and sizes_py[-1] == cap, (sizes_cpp, sizes_py)
    for a, b in zip(counts_cpp, counts_py):
        assert torch.equal(a, b), (a, b)
    assert int(counts_py[0][0]) >= 30
    worst = 0.0
    for a, b in zip(params_cpp, g.params()):
        worst = max(worst, float((a - b.detach()).abs().max()))
        assert torch.allclose(a, b.detach(), rtol=1e-4, atol=1e-6)
    print("measured: largest parameter difference C++ / Python after", steps, "steps with mcmc on:", worst)
    # ---- a process group is refused (the factored exchange stands for it: no second rank is needed to ask)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        ops.trainer_set_options(h, {"mcmc": 1.0})
        ops.trainer_set_factored_exchange(h, True)
        import pytest
        with pytest.raises(RuntimeError, match="mcmc_ is not supported with a process group"):
            ops.trainer_render_and_backward(h, *pg._cam_args(cam, dev), gt, mask)
    finally:
        ops.trainer_destroy(h)

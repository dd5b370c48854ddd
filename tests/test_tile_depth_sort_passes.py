"""csrc/tile_depth_sort.hip where its pass structure changes: 9-bit digits (one pass up to 9 bits of key span, two up to 18, three up
to 27, four beyond), and for lists in LDS with 19 .. 27 bits of span the two passes on the top 18 bits followed by the fix-up of the
runs of equal prefix, with the exact passes as the fallback when a run is longer than TDS_CAP.  Every list is compared, exactly,
with a stable argsort of its keys.  Run here on the wave64 emulator build; test_gpu_tile_depth_sort_passes.py runs the same cases on
the device."""
import numpy as np
import pytest
import torch

import stages

CPU = torch.device("cpu")
CAP = 8   # TDS_CAP of tile_depth_sort.hip: the longest run of equal 18-bit prefixes the fix-up ranks
LENGTHS = (2, 63, 64, 65, 255, 256, 257, 764, 2047, 2048, 2049, 5000)
SPANS = (1, 8, 9, 10, 17, 18, 19, 26, 27, 28, 32)
RUN_BITS = (19, 23, 27)   # 1, 5 and 9 bits below the 18-bit prefix
ONE = 0x3F800000          # the bits of 1.0f


def check_lists(lib_path, dev, key_lists, seed):
    """One launch over the given lists (each: its keys in arrival order).  The ids of a list ascend in arrival order, as the stable
    tile sort delivers them, and the lists' ids interleave."""
    rng = np.random.default_rng(seed)
    lengths = [len(k) for k in key_lists]
    P = int(sum(lengths))
    perm = rng.permutation(P)
    key = np.zeros(P, np.uint32)
    lists, at = [], 0
    for k in key_lists:
        ids = np.sort(perm[at:at + len(k)])
        key[ids] = np.asarray(k, np.uint32)
        lists.append(ids)
        at += len(k)
    pl = np.concatenate(lists).astype(np.uint32) if P else np.zeros(0, np.uint32)
    got = stages.tile_depth_sort(lib_path, dev, lengths, key, pl)
    at = 0
    for j, ids in enumerate(lists):
        want = ids[np.argsort(key[ids], kind="stable")]
        assert np.array_equal(got[at:at + len(ids)], want), (j, len(ids))
        at += len(ids)


def span_keys(rng, n, bits, base=None):
    """n keys whose largest and smallest differ in exactly `bits` bits"""
    if base is None:
        base = 0 if bits > 28 else ONE
    k = base + rng.integers(0, 1 << bits, n, dtype=np.uint64)
    at = rng.choice(n, 2, replace=False)
    k[at[0]] = base + (1 << bits) - 1
    k[at[1]] = base
    assert int(k.max() - k.min()).bit_length() == bits
    return k.astype(np.uint32)


def run_keys(rng, n, bits, runs, lows="random", base=ONE):
    """n keys spanning exactly `bits` (19 .. 27) bits whose 18-bit prefixes of key - min are all distinct, except that the prefix at
    sorted position s (of the distinct prefixes) holds a run of L entries for every (s, L) of `runs`; in random arrival order.  lows: the bits below the prefix
    inside a run -- random, all equal, or descending in arrival order (the fix-up then reverses the run; wrapping where the run is
    longer than the field, which leaves equal values too)."""
    low = bits - 18
    distinct = n - sum(L for _, L in runs) + len(runs)
    pre = np.sort(rng.choice(np.arange(1, (1 << 18) - 1), distinct - 2, replace=False))
    pre = np.concatenate([[0], pre, [(1 << 18) - 1]]).astype(np.uint64)
    runs = [(s % distinct, L) for s, L in runs]   # (a negative position counts from the end)
    rel, run_of, length = [], [], dict(runs)
    assert len(length) == len(runs)
    for s, p in enumerate(pre):
        L = length.get(s, 1)
        if L == 1:
            lo = rng.integers(0, 1 << low, 1, dtype=np.uint64)
        elif lows == "equal":
            lo = np.full(L, rng.integers(0, 1 << low), np.uint64)
        elif lows == "descending":
            lo = (np.arange(L, 0, -1, dtype=np.uint64) - 1) % np.uint64(1 << low)
        else:
            lo = rng.integers(0, 1 << low, L, dtype=np.uint64)
        if s == 0:
            lo[0 if lows == "equal" else -1:] = 0   # the smallest key has no low bits: the kernel's prefixes (of key - min) are these prefixes
        rel.append((p << np.uint64(low)) | lo)
        run_of.append(np.full(L, s))
    rel, run_of = np.concatenate(rel), np.concatenate(run_of)
    assert len(rel) == n and int(rel.max() - rel.min()).bit_length() == bits and rel.min() == 0
    # a random arrival order in which the entries of a run keep the order built above
    when = rng.permutation(n)
    for s, _ in runs:
        m = np.nonzero(run_of == s)[0]
        when[m] = np.sort(when[m])
    out = np.empty(n, np.uint64)
    out[when] = rel
    return (base + out).astype(np.uint32)


def run_lists(rng, bits):
    """runs of CAP - 1, CAP (both ranked by the fix-up), CAP + 1 and 300 entries (both fall back), two per list and far apart: the first
    across the 64-entry boundary of the first wave's first round, the second near the end"""
    out = []
    for L in (CAP - 1, CAP, CAP + 1, 300):
        for lows in ("random", "equal", "descending"):
            out.append(run_keys(rng, 764, bits, [(60, L), (-3, L)], lows))
    out.append(run_keys(rng, 2048, bits, [(0, CAP), (505, CAP), (1000, 2), (1001, 3), (1002, CAP)], "descending"))
    out.append(run_keys(rng, 2048, bits, [(2048 - CAP - 1, CAP + 1)], "random"))   # the only long run ends the list
    out.append(run_keys(rng, 65, bits, [(1, CAP), (2, CAP), (3, CAP)], "random"))
    out.append(run_keys(rng, 2 * CAP + 3, bits, [(1, CAP + 1), (2, CAP)], "descending"))
    return out


def special_lists(rng):
    """the bit patterns of +inf, a NaN and 0xFFFFFFFF among ordinary depths, several times each (ties keep arrival order)"""
    out = []
    for n, specials in ((764, (0x7F800000, 0x7FC00000, 0xFFFFFFFF)), (764, (0x7F800000, 0x7FC00000)), (3000, (0x7F800000, 0x7FC00000, 0xFFFFFFFF)),
                        (3, (0xFFFFFFFF, 0x7FC00000, 0x7F800000)), (64, (0xFFFFFFFF, 0))):
        k = (ONE + rng.integers(0, 1 << 24, n, dtype=np.uint64)).astype(np.uint32)
        at = rng.choice(n, min(n, 4 * len(specials)), replace=False)
        k[at] = np.resize(np.array(specials, np.uint32), len(at))
        out.append(k)
    return out


def case_lengths_at_span(lib_path, dev, bits):
    rng = np.random.default_rng(100 + bits)
    check_lists(lib_path, dev, [span_keys(rng, n, bits) for n in LENGTHS], bits)


def case_all_equal(lib_path, dev):
    check_lists(lib_path, dev, [np.full(n, v, np.uint32) for n in LENGTHS for v in (ONE, 0, 0xFFFFFFFF)], 1)


def case_runs(lib_path, dev, bits):
    check_lists(lib_path, dev, run_lists(np.random.default_rng(200 + bits), bits), bits)


def case_special_patterns(lib_path, dev):
    check_lists(lib_path, dev, special_lists(np.random.default_rng(3)), 3)


def case_mixed(lib_path, dev):
    rng = np.random.default_rng(4)
    lists = [np.zeros(0, np.uint32), np.full(1, ONE, np.uint32)]
    for bits in SPANS:
        lists += [span_keys(rng, int(n), bits) for n in rng.choice(LENGTHS, 3, replace=False)]
    for bits in RUN_BITS:
        lists += run_lists(rng, bits)[::3]
    lists += special_lists(rng)
    lists += [np.full(n, ONE, np.uint32) for n in (2, 257, 2049)]
    lists += [np.zeros(0, np.uint32), np.full(1, 7, np.uint32)]
    check_lists(lib_path, dev, [lists[i] for i in rng.permutation(len(lists))], 4)


@pytest.mark.parametrize("bits", SPANS)
def test_every_length_at_every_span(emu_lib_path, bits):
    case_lengths_at_span(emu_lib_path, CPU, bits)


def test_all_keys_equal(emu_lib_path):
    case_all_equal(emu_lib_path, CPU)


@pytest.mark.parametrize("bits", RUN_BITS)
def test_runs_of_equal_prefix(emu_lib_path, bits):
    case_runs(emu_lib_path, CPU, bits)


def test_special_bit_patterns(emu_lib_path):
    case_special_patterns(emu_lib_path, CPU)


def test_mixed_lists_in_one_launch(emu_lib_path):
    case_mixed(emu_lib_path, CPU)

#!/usr/bin/env python3
"""Counts, per kernel of a gfx950 assembly listing, the vector-memory loads and the waits on them.

  hipcc --offload-arch=gfx950 <the flags of CMakeLists.txt> -Iinclude --cuda-device-only -S -o bwd.s photo-slam_amd/csrc/preprocess_bwd.hip
  python tools/wait_chain.py bwd.s [substring of a kernel name ...]

A kernel whose time is latency (the per-Gaussian stages: EXPERIMENTS.md, "Per-Gaussian kernels: load chains") pays one HBM round
trip for every `s_waitcnt vmcnt(N)` that stands behind loads issued since the wait before it; loads issued back to back and
waited for once cost one.  Per kernel the table gives

  loads     global_load_* / buffer_load_* / flat_load_* instructions (scratch_load_* apart: `scratch`)
  stores    global_store_* / buffer_store_* / flat_store_*
  waits     s_waitcnt instructions with a vmcnt field
  trips     waits that have at least one load in front of them that no earlier wait stands behind: the static length of the
            kernel's chain of dependent round trips (a loop body counts once, whatever its trip count)
  ld/trip   loads per trip: how many loads a wait covers on average
  vgpr, lds, scratch, waves/SIMD   from the kernel's metadata: min(8, 512 / vgprs rounded up to 8, LDS-resident workgroups x waves
            per workgroup / 4 SIMDs) with 160 KiB of LDS per CU

Static counts of the listing, not a measurement: a predicated-off load still counts, and a wait inside a loop counts once.
"""
import re
import sys

LOAD = re.compile(r"^\s+(global_load|buffer_load|flat_load)_")
STORE = re.compile(r"^\s+(global_store|buffer_store|flat_store)_")
SCRATCH = re.compile(r"^\s+scratch_(load|store)_")
WAIT = re.compile(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)")
LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")
LDS_PER_CU = 160 * 1024


def kernels(lines):
    """name -> list of instruction lines, for every symbol that ends in s_endpgm"""
    out, name, body = {}, None, []
    for ln in lines:
        m = LABEL.match(ln)
        if m and not m.group(1).startswith((".L", "__hip")):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(ln)
        if ln.strip().startswith(".end_amdhsa_kernel") or ln.strip().startswith(".Lfunc_end"):
            if any("s_endpgm" in b for b in body):
                out.setdefault(name, body)
            name = None
    return out


def metadata(lines):
    """name -> {vgpr, lds, scratch, wg} from the amdhsa.kernels YAML at the end of the listing"""
    out, cur = {}, {}
    keys = {".vgpr_count": "vgpr", ".group_segment_fixed_size": "lds", ".private_segment_fixed_size": "scratch",
            ".max_flat_workgroup_size": "wg", ".name": "name"}
    for ln in lines:
        s = ln.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args"):
            if "name" in cur:
                out[cur["name"]] = cur
            cur = {}
        for k, v in keys.items():
            if s.lstrip("- ").startswith(k + ":"):
                val = s.split(":", 1)[1].strip()
                cur[v] = val if v == "name" else int(val)
    if "name" in cur:
        out[cur["name"]] = cur
    return out


def count(body):
    loads = stores = waits = trips = scratch = 0
    pending = 0   # loads issued since the last vmcnt wait
    for ln in body:
        if LOAD.match(ln):
            loads += 1
            pending += 1
        elif STORE.match(ln):
            stores += 1
        elif SCRATCH.match(ln):
            scratch += 1
        elif WAIT.match(ln):
            waits += 1
            if pending:
                trips += 1
            pending = 0
    return dict(loads=loads, stores=stores, waits=waits, trips=trips, scratch_ops=scratch)


def waves_per_simd(md):
    vg = max(8, (md.get("vgpr", 8) + 7) // 8 * 8)
    by_vgpr = min(8, 512 // vg)
    waves_per_wg = max(1, (md.get("wg", 64) + 63) // 64)
    lds = md.get("lds", 0)
    if lds:
        by_lds = (LDS_PER_CU // lds) * waves_per_wg / 4.0
        return min(float(by_vgpr), by_lds)
    return float(by_vgpr)


def short(name):
    try:
        import subprocess
        r = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True)
        d = r.stdout.strip() or name
    except OSError:
        d = name
    d = d.replace("void ", "").replace("gsr::", "")
    return d.split("(")[0]


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    lines = open(argv[1]).read().splitlines()
    want = argv[2:]
    ks, md = kernels(lines), metadata(lines)
    print(f"{'kernel':64s} {'loads':>5s} {'stores':>6s} {'waits':>5s} {'trips':>5s} {'ld/trip':>7s} {'vgpr':>4s} {'lds':>6s} {'scratch':>7s} {'waves/SIMD':>10s}")
    for name, body in ks.items():
        if name not in md:
            continue   # a device function, not a kernel
        label = short(name)
        if want and not any(w in label or w in name for w in want):
            continue
        c, m = count(body), md[name]
        per = c["loads"] / c["trips"] if c["trips"] else 0.0
        print(f"{label[:64]:64s} {c['loads']:5d} {c['stores']:6d} {c['waits']:5d} {c['trips']:5d} {per:7.1f} {m.get('vgpr', 0):4d} "
              f"{m.get('lds', 0):6d} {m.get('scratch', 0):7d} {waves_per_simd(m):10.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

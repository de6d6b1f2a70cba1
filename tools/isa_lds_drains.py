"""Diagnostic (no GPU needed): LDS reads that are drained one short group at a time.
A wave that waits with `s_waitcnt lgkmcnt(0)` between the LDS reads of one straight-line stretch pays a whole LDS round trip (about 50
cycles for a wave alone on its SIMD, more under occupancy) per wait; a counted wait, `lgkmcnt(N)` with N > 0, leaves the N youngest
reads in flight.  This script compiles kernel translation units to ISA and lists, per kernel and per straight-line run (basic block)
that holds at least --min-reads LDS reads: the reads, the full drains BETWEEN the first and the last read, the counted waits between
them and the smallest count among those.  It reads `ds_read*` and `s_waitcnt` lines only.
usage: python tools/isa_lds_drains.py [--min-reads N] [--kernel SUBSTRING] [--asm FILE.s | unit ...]   (default unit: k_scanw)
A drain in front of a dependent address (a table index read from LDS) is needed, and the counter is shared with scalar-memory loads: a
wait counted here may stand for an `s_load` issued in the same run, not for an LDS read.  Read the block before acting on a line."""
import argparse
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--min-reads", type=int, default=8)
ap.add_argument("--kernel", default="", help="only kernels whose demangled name contains this")
ap.add_argument("--asm", help="read this ISA file instead of compiling")
ap.add_argument("units", nargs="*")
args = ap.parse_args()


def isa_of(u):
    out = f"/tmp/isa_{u}.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-gpu-rdc",
                           "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "rabitq-rs_amd", "csrc", "device", u + ".hip")], stderr=subprocess.DEVNULL)
    return out


def lgkm(line):
    """the LDS counter a wait names (None: the wait does not name it)"""
    m = re.search(r"lgkmcnt\((\d+)\)", line)
    return int(m.group(1)) if m else None


for path in ([args.asm] if args.asm else [isa_of(u) for u in (args.units or ["k_scanw"])]):
    for f in re.split(r"\n(?=_ZN3rbq[\w]+:\s)", open(path).read()):
        name = f.split(":")[0]
        if not name.startswith("_ZN3rbq"):
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"\(.*", "", dem).replace("void rbq::", "").replace("rbq::", "")
        if args.kernel not in dem:
            continue
        lines = f.split("\n")
        lines = lines[:next((i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")), len(lines))]
        # straight-line runs: a label or a branch ends one
        runs, cur, label = [], [], "entry"
        for l in lines[1:]:
            s = l.strip()
            if re.match(r"^\.LBB\d+_\d+:", l):
                runs.append((label, cur)); cur, label = [], l.split(":")[0]
            elif s.startswith(("ds_read", "s_waitcnt")):
                cur.append(s)
            elif s.startswith(("s_cbranch", "s_branch")):
                runs.append((label, cur)); cur, label = [], label + "+"
        runs.append((label, cur))
        tot_reads = tot_drains = tot_counted = 0
        rows = []
        for label, body in runs:
            rd = [i for i, x in enumerate(body) if x.startswith("ds_read")]
            if len(rd) < args.min_reads:
                continue
            waits = [lgkm(x) for x in body[rd[0]:rd[-1]] if x.startswith("s_waitcnt")]
            waits = [w for w in waits if w is not None]
            drains, counted = sum(1 for w in waits if w == 0), [w for w in waits if w > 0]
            kinds = sorted({body[i].split()[0] for i in rd})
            rows.append(f"    {label:12s} reads {len(rd):4d}  drains {drains:3d}  counted waits {len(counted):3d}"
                        f"  (smallest N {min(counted) if counted else '-'})  {' '.join(kinds)}")
            tot_reads += len(rd); tot_drains += drains; tot_counted += len(counted)
        print(f"{dem}: {tot_reads} reads, {tot_drains} drains, {tot_counted} counted waits in {len(rows)} runs")
        for r in rows:
            print(r)

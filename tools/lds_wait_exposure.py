#!/usr/bin/env python3
"""How far behind their producing read the LDS waits of a gfx950 .s file stand.

With one wavefront per SIMD a `s_waitcnt lgkmcnt(n)` that follows the `ds_read*` it waits for by a few
instructions is an exposed LDS round trip: nothing else runs meanwhile.  For every kernel of the file, split at
the header and the back-edge of its iteration loop (the last loop of 500 instructions or more; a kernel without
one is one region),
this prints

    LDS waits <= 10 instructions behind their read | <= 2 behind | all LDS waits

and the same for `vmcnt` waits against `global_load*`, plus the number of those that stand directly (<= 2
instructions) behind a load that is the only one they wait for -- a memory round trip paid on its own.

The counters retire in order, so `lgkmcnt(n)` waits for everything but the n youngest LGKM operations in flight;
the read a wait "waits for" is the youngest `ds_read*` among those.  A wait that retires no read is not counted.
Only `ds_*`, scalar loads (they share the counter), `global_*` / `scratch_*` / `buffer_*` and `s_waitcnt` are
looked at; the walk is in layout order and ignores branches, which is exact for the straight-line code of the
fully unrolled kernels.

    usage: lds_wait_exposure.py file.s [--near 10] [--tight 2] [--marks]

--marks splits the regions further at `; DQPMARK n` comments (-DDQP_MARKS builds).
"""
import argparse
import re
import subprocess


def kernels(lines):
    """-> [(name, first line, last line)] of the functions that end in s_endpgm"""
    out, name, start = [], None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and not m.group(1).startswith((".L", "__hip")):
            name, start = m.group(1), i
        elif l.startswith(".Lfunc_end") and name:
            if any("s_endpgm" in x for x in lines[start:i]):
                out.append((name, start, i))
            name = None
    return out


def largest_loop(lines, a, b, min_insns=500):
    labels = {}
    for i in range(a, b):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            labels[m.group(1)] = i
    # the iteration is the last loop of that size in layout order (block placement can leave an unconditional
    # backward branch over a stretch of the setup in front of it); its outermost back-edge counts
    best = None
    for i in range(a, b):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            h = labels[m.group(1)]
            if sum(is_insn(l.strip()) for l in lines[h:i]) < min_insns:
                continue
            if best is None or h > best[1] or (h <= best[0] and i >= best[1]):
                best = (h, i)
    return best


def is_insn(t):
    return bool(t) and not t.startswith((";", ".", "//")) and not t.endswith(":")


def count(t, name, default):
    m = re.search(name + r"\((\d+)\)", t)
    return int(m.group(1)) if m else default


class Region:
    def __init__(self, name):
        self.name = name
        self.lds = [0, 0, 0]     # near, tight, all
        self.vm = [0, 0, 0, 0]   # near, tight, all, single load directly in front


def walk(lines, a, b, cuts, near, tight, marks):
    """cuts: sorted [(line, region name)]; -> [Region]"""
    regions = [Region(cuts[0][1])]
    nxt = 1
    lgkm, vm = [], []            # in flight, oldest first: (instruction index, is a read/load)
    n = 0
    for i in range(a, b):
        while nxt < len(cuts) and i >= cuts[nxt][0]:
            regions.append(Region(cuts[nxt][1]))
            nxt += 1
        t = lines[i].strip()
        if marks:
            m = re.match(r";\s*DQPMARK\s+(\d+)", t)
            if m:
                regions.append(Region(regions[-1].name.split(" @")[0] + " @mark " + m.group(1)))
        if not is_insn(t):
            continue
        n += 1
        op = t.split()[0]
        reg = regions[-1]
        if op.startswith("ds_"):
            lgkm.append((n, op.startswith("ds_read") or op.startswith("ds_load")))
        elif op.startswith(("s_load", "s_buffer_load", "s_scratch_load")):
            lgkm.append((n, False))
        elif op.startswith(("global_", "scratch_", "buffer_", "flat_")):
            vm.append((n, op.startswith("global_load")))
            if op.startswith("flat_"):
                lgkm.append((n, False))
        elif op == "s_waitcnt":
            raw = re.fullmatch(r"s_waitcnt\s+(\d+|0x[0-9a-fA-F]+)", t)
            keep_l = 0 if raw else count(t, "lgkmcnt", None)
            keep_v = 0 if raw else count(t, "vmcnt", None)
            if keep_l is not None and len(lgkm) > keep_l:
                done, lgkm = lgkm[:len(lgkm) - keep_l], lgkm[len(lgkm) - keep_l:]
                reads = [k for k, rd in done if rd]
                if reads:
                    d = n - reads[-1]
                    reg.lds[2] += 1
                    reg.lds[0] += d <= near
                    reg.lds[1] += d <= tight
            if keep_v is not None and len(vm) > keep_v:
                done, vm = vm[:len(vm) - keep_v], vm[len(vm) - keep_v:]
                loads = [k for k, ld in done if ld]
                if loads:
                    d = n - loads[-1]
                    reg.vm[2] += 1
                    reg.vm[0] += d <= near
                    reg.vm[1] += d <= tight
                    reg.vm[3] += len(loads) == 1 and d <= tight
    return regions


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--near", type=int, default=10)
    ap.add_argument("--tight", type=int, default=2)
    ap.add_argument("--marks", action="store_true")
    args = ap.parse_args()
    lines = open(args.asm).read().split("\n")
    for name, a, b in kernels(lines):
        try:
            pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        except OSError:
            pretty = name
        print(pretty[:110])
        loop = largest_loop(lines, a, b)
        if loop:
            cuts = [(a, "setup (entry -> loop header)"), (loop[0], "loop (one iteration)"),
                    (loop[1] + 1, "epilogue (loop exit -> end)")]
        else:
            cuts = [(a, "whole kernel")]
        print("  %-36s | LDS <=%d  <=%d  all | vmcnt <=%d  <=%d  all  single" %
              ("region", args.near, args.tight, args.near, args.tight))
        for reg in walk(lines, a, b, cuts, args.near, args.tight, args.marks):
            print("  %-36s | %6d %4d %4d | %8d %4d %4d %7d" % ((reg.name,) + tuple(reg.lds) + tuple(reg.vm)))


if __name__ == "__main__":
    main()

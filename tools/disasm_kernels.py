#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds of one object (tools/disasm_diff.sh diffs the whole
object, which a build that ADDS kernels always changes): every function present in both is compared instruction by
instruction with the addresses stripped, new and removed ones are listed, and the scratch / VGPR metadata of the new
ones is printed next to that of the old function they were derived from (same name without the StridedBounds<> wrapper).
usage: tools/disasm_kernels.py old.o new.o   (no GPU needed)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(obj, td, tag):
    fat, co = os.path.join(td, tag + ".fat"), os.path.join(td, tag + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    return co


def functions(co):
    """{demangled name: [instruction lines]}"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co],
                         capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
        if m:
            cur = out.setdefault(strip_params(m.group(1)), [])
        elif cur is not None and line.strip() and line.strip() != "...":
            cur.append(re.sub(r"<[^>]*\+0x[0-9a-f]+>", "", re.sub(r" *//.*$", "", line)).strip())
    return out


def metadata(co):
    """{demangled name: (vgpr, scratch bytes, lds bytes)}"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        name = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
        out[strip_params(name)] = (g("vgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    return out


def strip_params(name):
    """the function's name without its parameter list (a kernel's argument struct may be spelled through a type alias)"""
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(name[i], 0)
            if depth == 0:
                name = name[:i]
                break
    # a kernel that became a template on the layout alone: its vector instantiation is the old kernel
    return re.sub(r"^void (.*_kernel)<false>$", r"\1", name.replace(" >", ">"))


def unwrap(name):
    """the name with every StridedBounds<X> replaced by X"""
    name = re.sub(r"^void (.*_kernel)<true>$", r"\1", name)
    key = "StridedBounds<"
    while key in name:
        i = name.index(key)
        start = max(name.rfind("<", 0, i), name.rfind(",", 0, i), name.rfind(" ", 0, i)) + 1
        j, depth = i + len(key), 1
        while depth:
            depth += {"<": 1, ">": -1}.get(name[j], 0)
            j += 1
        name = name[:start] + name[i + len(key):j - 1].strip() + name[j:]
    return name


def main(old, new):
    with tempfile.TemporaryDirectory() as td:
        co_o, co_n = code_object(old, td, "old"), code_object(new, td, "new")
        fo, fn, mo, mn = functions(co_o), functions(co_n), metadata(co_o), metadata(co_n)
    same = [k for k in fo if k in fn and fo[k] == fn[k]]
    diff = [k for k in fo if k in fn and fo[k] != fn[k]]
    print("%d functions in both: %d identical, %d differ; %d new, %d removed" % (
        len(same) + len(diff), len(same), len(diff), len(set(fn) - set(fo)), len(set(fo) - set(fn))))
    for k in diff:
        print("DIFFERS  %s  (%d -> %d instructions)" % (k, len(fo[k]), len(fn[k])))
    for k in sorted(set(fo) - set(fn)):
        print("REMOVED  %s" % k)
    for k in sorted(set(fn) - set(fo)):
        base = unwrap(k)
        b = mo.get(base) or mn.get(base)
        print("NEW      %s\n         vgpr/scratch/lds %s   base %s   instructions %d (base %s)" % (
            k, mn.get(k), b, len(fn[k]), len(fn.get(base, fo.get(base, []))) or "?"))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))

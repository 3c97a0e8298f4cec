#!/usr/bin/env python3
"""Is the gfx950 device code of this tree the same as another checkout's?  For a change that touches host code only.
    python tools/device_code_diff.py ../parent-checkout > profiles/rNN_device_code.txt
    python tools/device_code_diff.py ../parent-checkout imp_geom.hip imp_resize.hip      # those files only
Compiles every .hip under csrc/ of both trees as tools/kernel_resources.py does (hipcc -S --cuda-device-only, no GPU
needed), cuts the assembly into functions by symbol and compares them as text, kernel by kernel.  The order of functions in
a file follows the order host code instantiates them in and may move: it is ignored, and so are the numbers it gives to local
labels (.LBB<n>_, .Lfunc_end<n>, ..., and BB<n>_ in the comments, whose column moves with them) and the __hip_cuid_* lines.  Exit status 1 when a kernel is missing, new or different."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def functions(root, f):
    with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-fno-fast-math", "-I", os.path.join(root, "include"), "-S", "--cuda-device-only", "-o", tmp.name,
                               os.path.join(root, "ngx_http_imgproc_amd", "csrc", f)], stderr=subprocess.DEVNULL)
        lines = open(tmp.name).read().split("\n")
    out, name, ended = {}, None, False
    for l in lines:
        m = re.search(r"; -- Begin function (\S+)", l)
        if m:
            name, ended = m.group(1), False
            out[name] = []
        elif name and ended and not (l.startswith("\t.set ") or l.startswith(";") or ".AMDGPU.csdata" in l):
            name = None                                 # past the function's resource summary
        if name:
            out[name].append(re.sub(r"\s+;", " ;", re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+", r"\1", l)))
            ended = ended or "; -- End function" in l
    return {k: "\n".join(v) for k, v in out.items()}


def main():
    other, only = sys.argv[1], sys.argv[2:]
    files = sorted(f for f in os.listdir(os.path.join(HERE, "ngx_http_imgproc_amd", "csrc")) if f.endswith(".hip") and (not only or f in only))
    with ThreadPoolExecutor(max_workers=8) as pool:
        mine = list(pool.map(lambda f: functions(HERE, f), files))
        theirs = list(pool.map(lambda f: functions(other, f), files))
    bad = 0
    print("%-20s %8s %8s  %s" % ("file", "kernels", "other", "verdict"))
    for f, a, b in zip(files, mine, theirs):
        ka = {k for k, v in a.items() if ".amdhsa_kernel" in v}
        kb = {k for k, v in b.items() if ".amdhsa_kernel" in v}
        diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        gone, new = sorted(set(b) - set(a)), sorted(set(a) - set(b))
        print("%-20s %8d %8d  %s" % (f, len(ka), len(kb), "identical" if not (diff or gone or new) else "DIFFERENT"))
        for tag, names in (("differs", diff), ("missing here", gone), ("only here", new)):
            for k in names:
                print("    %s: %s" % (tag, k))
        bad += len(diff) + len(gone) + len(new)
    print("every function of every file identical" if not bad else "%d functions differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

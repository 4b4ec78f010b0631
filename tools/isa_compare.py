"""Compare the gfx950 device code of surikatoko_amd/csrc/srk_ba_kernels.hip at a git revision with the working tree, kernel by
kernel (instruction text; labels and symbol names normalised).  Kernels that gained a frame-variable template parameter are
matched with FV = 10 (the default layout) against the revision's kernel of the same name.  Host only: needs hipcc and git.

    python tools/isa_compare.py [REV] [--allow-missing NAME ...]        (REV defaults to HEAD)
Prints one line per kernel that differs and a summary; exit status 0 when every kernel of REV has an identical counterpart and
the working tree instantiates nothing that REV did not.  A kernel of REV without a counterpart is an error unless its function
name is given with --allow-missing (a kernel taken out on purpose): it is then printed as "retired" and counted apart.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "surikatoko_amd/csrc"
FILES = ["srk_ba_kernels.hip", "srk_dev.hpp", "srk_geom.hpp", "srk_step_tables.inc"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "--cuda-device-only", "-S"]


def device_asm(src_dir, out):
    subprocess.run([HIPCC, *FLAGS, os.path.join(src_dir, "srk_ba_kernels.hip"), "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernels(lines):
    out, cur, body = {}, None, []
    for line in lines:
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            if cur:
                out[cur] = body
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end") or re.match(r"\s*\.section", line):
            out[cur], cur = body, None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip() or s.strip().startswith("."):
            continue
        body.append(re.sub(r"_Z\S+", "SYM", re.sub(r"\.LBB\d+_\d+", "L", s)))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, r))


def key(name):
    # FV = 10 instantiations of kernels that were made templates on the frame-variable count
    name = re.sub(r", 10>", ">", name)
    name = re.sub(r"^void (\w+)<10>\(", r"\1(", name)
    return name


def function_name(demangled):
    m = re.match(r"^(?:void )?(\w+)", demangled)
    return m.group(1) if m else demangled


def main():
    args, allowed = sys.argv[1:], set()
    while "--allow-missing" in args:
        i = args.index("--allow-missing")
        if i + 1 >= len(args):
            sys.exit("--allow-missing needs a kernel's function name")
        allowed.add(args[i + 1])
        del args[i:i + 2]
    rev = args[0] if args else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        old_dir = os.path.join(tmp, "old")
        os.makedirs(old_dir)
        for f in FILES:
            with open(os.path.join(old_dir, f), "w") as fh:
                fh.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{CSRC}/{f}"], check=True, capture_output=True,
                                        text=True).stdout)
        old = kernels(device_asm(old_dir, os.path.join(tmp, "old.s")))
        new = kernels(device_asm(os.path.join(ROOT, CSRC), os.path.join(tmp, "new.s")))
    dold, dnew = demangle(list(old)), demangle(list(new))
    new_by_key = {key(dnew[k]): k for k in new}
    same, bad, retired = 0, 0, 0
    for k in old:
        nk = new_by_key.get(key(dold[k]))
        if nk is None and function_name(dold[k]) in allowed:
            print("retired :", dold[k][:150])
            retired += 1
        elif nk is None:
            print("missing :", dold[k][:150])
            bad += 1
        elif old[k] == new[nk]:
            same += 1
        else:
            n_diff = sum(1 for a, b in zip(old[k], new[nk]) if a != b) + abs(len(old[k]) - len(new[nk]))
            print(f"differs : {dold[k][:110]}  ({len(old[k])} -> {len(new[nk])} instructions, {n_diff} lines differ)")
            bad += 1
    old_keys = {key(dold[k]) for k in old}
    added = sorted(k for k in new_by_key if k not in old_keys)
    for k in added:
        print("new     :", k[:150])
    print(f"{same} of {len(old) - retired} kernels of {rev} identical in the working tree ({retired} retired); "
          f"{len(added)} new instantiations")
    return 0 if bad == 0 and not added else 1


if __name__ == "__main__":
    sys.exit(main())

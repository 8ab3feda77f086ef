"""Device code of two trees of this repository compared without a GPU.

    python tools/device_asm_diff.py PARENT_ROOT NEW_ROOT FILE.hip [FILE.hip ..] [--log FILE]

PARENT_ROOT is a checkout of the parent commit (`git archive <commit> | tar -x -C DIR`),
NEW_ROOT this tree. Each FILE of csrc/ is compiled in both trees with the flags its own Makefile
gives that file (read from `make -n`), plus `--cuda-device-only -S`, from csrc/ of the tree so
the relative path is the same in both. Per kernel the body (its label to its last instruction; comments,
blank lines and section / alignment directives dropped; the kernel's own mangled name and the
function index in its labels normalised) and the .amdhsa_kernel resource block are compared and
reported as IDENTICAL, DIFFERENT (with the resource fields that changed), ONLY IN PARENT or
ONLY IN NEW. Kernels are matched by demangled name. It diffs; it looks for nothing in particular.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join("rp-style-transfer_amd", "csrc")


def compile_asm(root: str, name: str, out: str) -> None:
    """FILE -> device assembly with the Makefile's flags for build/<stem>.o."""
    csrc = os.path.join(root, CSRC)
    obj = f"build/{os.path.splitext(name)[0]}.o"
    dry = subprocess.run(["make", "-n", "-B", obj], cwd=csrc, check=True, capture_output=True,
                         text=True).stdout
    line = next(l for l in dry.splitlines() if f"-c {name}" in l)
    cmd = shlex.split(line)
    i = cmd.index("-c")
    cmd[i:] = ["--cuda-device-only", "-S", name, "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cand = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin",
                            "llvm-cxxfilt")
        tool = cand if os.path.exists(cand) else None
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d).replace("rpst::", "").replace("(anonymous namespace)::", "")
        short[n] = d
    return short


def kernels(path: str):
    """{demangled name: (body lines, resource lines)} of one assembly file."""
    text = open(path).read().splitlines()
    names = [l.split()[1] for l in text if l.strip().startswith(".amdhsa_kernel ")]
    short = demangle(names)
    out = {}
    for name in names:
        start = text.index(next(l for l in text if l.startswith(name + ":")))
        # the resource block sits between the last instruction and .Lfunc_end
        r0 = next(i for i in range(start, len(text)) if text[i].strip() == f".amdhsa_kernel {name}")
        r1 = next(i for i in range(r0, len(text)) if text[i].strip() == ".end_amdhsa_kernel")
        end = r0

        def norm(line):
            line = line.split(";")[0].rstrip()
            line = line.replace(name, "KERNEL").replace(name[2:], "KERNEL")
            return re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+", r".L\1", line)

        body = [norm(l) for l in text[start:end]]
        body = [l for l in body if l.strip() and not re.match(r"\s*\.(section|p2align|text)\b", l)]
        res = [norm(l).strip() for l in text[r0 + 1:r1]]
        out[short[name]] = (body, [l for l in res if l])
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+", help="file names under csrc/, e.g. rpst_wct.hip")
    ap.add_argument("--log", default=None, help="also append the report to this file")
    a = ap.parse_args()
    log = open(a.log, "a") if a.log else None

    def say(line=""):
        print(line, flush=True)
        if log:
            log.write(line + "\n")

    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.files:
            asm = []
            for tag, root in (("parent", a.parent), ("new", a.new)):
                path = os.path.join(tmp, f"{tag}.{name}.s")
                compile_asm(os.path.abspath(root), name, path)
                asm.append(kernels(path))
            old, new = asm
            say(f"== {name}")
            same = diff = 0
            for k in sorted(set(old) | set(new)):
                if k not in new:
                    say(f"ONLY IN PARENT   {k}")
                elif k not in old:
                    say(f"ONLY IN NEW      {k}")
                elif old[k] == new[k]:
                    same += 1
                    say(f"IDENTICAL        {k} ({len(new[k][0])} lines)")
                else:
                    diff += 1
                    ops = list(difflib.unified_diff(old[k][0], new[k][0], lineterm="", n=0))
                    plus = sum(l.startswith("+") and not l.startswith("+++") for l in ops)
                    minus = sum(l.startswith("-") and not l.startswith("---") for l in ops)
                    say(f"DIFFERENT        {k} ({len(old[k][0])} -> {len(new[k][0])} lines, "
                        f"+{plus} -{minus})")
                    ro, rn = dict(l.split(None, 1) for l in old[k][1] if " " in l), \
                        dict(l.split(None, 1) for l in new[k][1] if " " in l)
                    changed = [f"{f} {ro.get(f)} -> {rn.get(f)}" for f in sorted(set(ro) | set(rn))
                               if ro.get(f) != rn.get(f)]
                    say("                 resources: " + ("; ".join(changed) if changed else "same"))
            say(f"identical {same}, different {diff}")
            say()
            status |= diff != 0
    return status


if __name__ == "__main__":
    sys.exit(main())

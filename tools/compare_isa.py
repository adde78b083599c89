"""Are the device kernels of two source trees the same machine code?

    python tools/compare_isa.py <git-commit>            # that commit's csrc/ against the working tree

Compiles every translation unit of ttt-video-dit_amd/csrc (the *.hip files present in both trees, with the flags of csrc/build.sh) to
gfx950 assembly (device only) in both trees and compares the instruction streams kernel by kernel (labels normalised, comments
dropped).  Used to show that a refactor - e.g. dropping a template parameter that has one instantiation left - leaves the code of
every kernel bit-for-bit alone when no GPU is at hand to re-run the parity tests.  A kernel whose stream is found under another name
(its template arguments changed) is reported as "identical, now named ..."; exit status 1 if any kernel changed or disappeared.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("ttt-video-dit_amd", "csrc")


def build_flags():
    """FLAGS of csrc/build.sh, so that both trees are compiled the way the library is."""
    m = re.search(r'^FLAGS="([^"]*)"', open(os.path.join(ROOT, CSRC, "build.sh")).read(), flags=re.M)
    return m.group(1).split()


def asm(src_dir, unit, out, flags):
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", unit + ".hip", "-o", out],
                   cwd=src_dir, stderr=subprocess.DEVNULL, check=True)
    text = open(out).read()
    functions = set(re.findall(r"^\s*\.type\s+(_Z\w+),@function", text, flags=re.M))      # (not the __device__ variables)
    kernels, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1) if m.group(1) in functions else None
            if cur is not None:
                kernels[cur] = []
        elif cur is not None:
            if "s_endpgm" in line:
                cur = None
                continue
            t = re.sub(r";.*", "", line).strip()
            if t and not t.startswith("."):
                kernels[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return kernels


def main():
    commit = sys.argv[1]
    flags = build_flags()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(f"git -C {ROOT} archive {commit} {CSRC} include | tar -x -C {tmp}", shell=True, check=True)
        old_dir, new_dir = os.path.join(tmp, CSRC), os.path.join(ROOT, CSRC)
        names = lambda d: {os.path.basename(f)[:-4] for f in glob.glob(os.path.join(d, "*.hip"))}
        units = sorted(names(old_dir) & names(new_dir))
        for unit in sorted(names(old_dir) ^ names(new_dir)):
            print(f"{unit}: not in both trees, skipped")
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = {(unit, d): pool.submit(asm, d, unit, os.path.join(tmp, f"{unit}.{tag}.s"), flags)
                    for unit in units for tag, d in (("a", old_dir), ("b", new_dir))}
        changed = 0
        for unit in units:
            a, b = jobs[unit, old_dir].result(), jobs[unit, new_dir].result()
            by_code = {tuple(v): k for k, v in b.items()}
            for k, v in a.items():
                if k in b and b[k] == v:
                    continue
                if tuple(v) in by_code:
                    print(f"{unit}: {k} identical, now named {by_code[tuple(v)]}")
                else:
                    print(f"{unit}: {k} CHANGED" if k in b else f"{unit}: {k} removed / changed under another name")
                    changed += 1
            print(f"{unit}: {len(a)} kernels compared, {max(len(b) - len(a), 0)} new")
        print("no kernel of the old tree changed" if not changed else f"{changed} kernel(s) changed")
        return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Does a change leave the device code as it was?  Compiles every .hip file under madrigal_amd/csrc of two source trees to gfx950
assembly with the build's own flags (madrigal_amd.build.FLAGS plus --cuda-device-only -S) and compares the text, file by file.

    python scripts/kernel_text_diff.py                      # the working tree against HEAD
    python scripts/kernel_text_diff.py --rev HEAD~1         # ... against another commit
    python scripts/kernel_text_diff.py --old DIR --new DIR  # two trees on disk
    python scripts/kernel_text_diff.py ensemble.hip ensemble_topk.hip       # these files only

The old tree is `git archive` of --rev, unpacked into a temporary directory.  Before the compare, comment lines, .file / .ident lines
and lines that name the per-translation-unit __hip_cuid_ symbol are dropped; the rest is compared whole -- the assembly carries every
kernel's register, scratch and LDS figures, so "identical" covers occupancy as well as the instruction stream.  Nothing in particular
is searched for.  CPU only: hipcc cross-compiles, no GPU is touched.  Exit status 0 when every file is identical."""
from __future__ import annotations

import argparse
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madrigal_amd import build as mdg_build  # noqa: E402  (the flags are imported, not copied)

CSRC = os.path.join("madrigal_amd", "csrc")
_FUNCTION = re.compile(r"\s*\.type\s+(\S+),@function")


def unpack_rev(rev: str, dest: str) -> None:
    """csrc and include of commit ``rev`` into ``dest``."""
    tar = subprocess.run(["git", "-C", ROOT, "archive", "--format=tar", rev, CSRC, "include"], check=True, capture_output=True).stdout
    with tarfile.open(fileobj=io.BytesIO(tar)) as t:
        t.extractall(dest)


def flags_for(tree: str) -> list:
    """The build's flags with its include directory replaced by ``tree``'s."""
    return [os.path.join(tree, "include") if f == mdg_build.INCLUDE else f for f in mdg_build.FLAGS]


def assembly(tree: str, src: str, out: str) -> str:
    """Device assembly of ``tree``'s ``src`` -> its text ('' if the tree has no such file)."""
    path = os.path.join(tree, CSRC, src)
    if not os.path.exists(path):
        return ""
    r = subprocess.run([mdg_build.HIPCC, *flags_for(tree), "--cuda-device-only", "-S", path, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {path}:\n{r.stdout}\n{r.stderr}")
    with open(out) as f:
        return f.read()


def kept_lines(text: str) -> list:
    keep = []
    for line in text.splitlines():
        s = line.strip()
        if not s or s.startswith(";") or s.startswith("//") or s.startswith(".file") or s.startswith(".ident") or "__hip_cuid_" in s:
            continue
        keep.append(line.rstrip())
    return keep


def first_difference(old: list, new: list) -> str:
    """The function the first differing line belongs to, and that place as a unified diff."""
    n = next((i for i, (a, b) in enumerate(zip(old, new)) if a != b), min(len(old), len(new)))
    name = "(before the first function)"
    for line in new[:n + 1]:
        m = _FUNCTION.match(line)
        if m:
            name = m.group(1)
    lo = max(0, n - 3)
    hunk = list(difflib.unified_diff(old[lo:n + 8], new[lo:n + 8], "old", "new", lineterm="", n=3))
    return f"first difference in {name} (kept line {n + 1}; {len(old)} lines old, {len(new)} new)\n    " + "\n    ".join(hunk)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", help=".hip file names under madrigal_amd/csrc (default: every one in either tree)")
    ap.add_argument("--rev", default="HEAD", help="commit whose tree is the old side (default HEAD)")
    ap.add_argument("--old", help="old tree on disk, instead of --rev")
    ap.add_argument("--new", default=ROOT, help="new tree (default: this checkout's working tree)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="kernel_text_diff_") as tmp:
        old = a.old
        if old is None:
            old = os.path.join(tmp, "old_tree")
            os.makedirs(old)
            unpack_rev(a.rev, old)
        listed = lambda tree: {f for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith(".hip")}    # noqa: E731
        files = sorted(a.files or (listed(old) | listed(a.new)))

        def one(src: str):
            o = kept_lines(assembly(old, src, os.path.join(tmp, "old_" + src[:-4] + ".s")))
            n = kept_lines(assembly(a.new, src, os.path.join(tmp, "new_" + src[:-4] + ".s")))
            return src, o, n

        different = 0
        with ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
            for src, o, n in ex.map(one, files):
                if o == n:
                    print(f"identical  {src}  ({len(n)} lines)", flush=True)
                    continue
                different += 1
                if not o or not n:
                    print(f"DIFFERENT  {src}  (only in the {'new' if n else 'old'} tree)", flush=True)
                else:
                    print(f"DIFFERENT  {src}  {first_difference(o, n)}", flush=True)
    print(f"{len(files) - different} of {len(files)} files identical" + ("" if not different else f", {different} DIFFERENT"))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())

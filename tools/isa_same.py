"""Is the device code of csrc/ the same as at another commit?  Needs hipcc, no GPU.

    python tools/isa_same.py [--base REV] [--flags="-DCIPS3D_STAMPS ..."] [--jobs N] [file.hip ...]

Compiles every csrc/*.hip (or the named ones) of REV (default HEAD) and of the working tree to gfx950 assembly with the
library's flags (build.FLAGS, build.FILE_FLAGS, --flags on top) and compares the kernels by mangled name.  One line per
translation unit, then the kernels that differ and those only one side has.  Exit status 1 if a kernel both sides have
differs or the working tree has one that REV has not.
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cips_3dplusplus_amd import build  # noqa: E402

# what differs between two compilations of one source, or moves when a neighbouring kernel goes: the compiler's comments, the
# per-file unique id, the function number inside local labels
NORMALISE = [(r"[ \t]*;.*$", ""), (r"__hip_cuid_[0-9a-f]+", "__hip_cuid_"), (r"\.L([A-Za-z_]+?)\d+(_\d+)?\b", r".L\1\2")]


def kernels(csrc, name, extra, out):
    """{mangled name: body + kernel descriptor} of every function of one translation unit."""
    cmd = [build.hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(name, []), *extra, "--cuda-device-only", "-S",
           os.path.join(csrc, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {csrc}/{name}:\n{r.stderr}")
    with open(out) as fh:
        asm = fh.read()
    for rx, to in NORMALISE:
        asm = re.sub(rx, to, asm, flags=re.M)
    found = {m.group(1): m.group(2) for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end:\n", asm, re.S | re.M)}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel\n", asm, re.S | re.M):
        found[m.group(1)] = found.get(m.group(1), "") + m.group(2)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--flags", default="")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    bad = False
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, "cips_3dplusplus_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old_csrc = os.path.join(tmp, "cips_3dplusplus_amd", "csrc")
        names = a.files or sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
        one = lambda n: (n, kernels(old_csrc, n, a.flags.split(), os.path.join(tmp, n + ".old.s")),      # noqa: E731
                         kernels(build.CSRC, n, a.flags.split(), os.path.join(tmp, n + ".new.s")))
        with cf.ThreadPoolExecutor(max_workers=a.jobs) as ex:
            for name, old, new in ex.map(one, names):
                lists = {"differs": sorted(k for k in new if k in old and new[k] != old[k]), "new": sorted(set(new) - set(old)),
                         "gone": sorted(set(old) - set(new))}
                bad = bad or bool(lists["differs"] or lists["new"])
                verdict = "same" if not any(lists.values()) else ", ".join(f"{len(v)} {k}" for k, v in lists.items())
                print(f"{name:22s} {len(old):4d} -> {len(new):4d} kernels  {verdict}")
                for tag, ks in lists.items():
                    for k in ks:
                        print(f"    {tag}: {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Is the device code of csrc/ the same as at another commit?  Needs hipcc, no GPU.

    python tools/isa_same.py [--base REV] [--flags="-DCIPS3D_STAMPS ..."] [--jobs N] [file.hip ...]

Compiles every csrc/*.hip (or the named ones, where a side has them) of REV (default HEAD) and of the working tree to gfx950
assembly with the library's flags (build.FLAGS, build.FILE_FLAGS, --flags on top), pools the kernels of all translation units
of each side by mangled name and compares the two pools: a kernel that moved to another file with its body unchanged is the
same.  One line per translation unit, one for the pools, then the kernels that differ and those only one side has.  Exit status 1
if a kernel both sides have differs, the working tree has one that REV has not, or the working tree defines a name in more
files than REV does (a copy).
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


def pool(units):
    """{mangled name: [(file, text), ...]} over the translation units of one side.  A kernel with internal linkage that a shared
    header defines may be compiled into more than one of them (vgg_shared.h): the copies are kept, sorted by text."""
    pooled = {}
    for name, found in sorted(units.items()):
        for k, text in found.items():
            pooled.setdefault(k, []).append((name, text))
    return {k: sorted(v, key=lambda ft: ft[1]) for k, v in pooled.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--flags", default="")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, "cips_3dplusplus_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        dirs = {"old": os.path.join(tmp, "cips_3dplusplus_amd", "csrc"), "new": build.CSRC}
        jobs = [(side, f) for side, d in dirs.items() for f in sorted(os.listdir(d))
                if f.endswith(".hip") and (not a.files or f in a.files)]
        one = lambda j: (j, kernels(dirs[j[0]], j[1], a.flags.split(), os.path.join(tmp, f"{j[1]}.{j[0]}.s")))   # noqa: E731
        units = {"old": {}, "new": {}}
        with cf.ThreadPoolExecutor(max_workers=a.jobs) as ex:
            for (side, name), found in ex.map(one, jobs):
                units[side][name] = found
    old, new = pool(units["old"]), pool(units["new"])
    texts = lambda copies: [t for _, t in copies]                                                                # noqa: E731
    files = lambda k: {f for side in (old, new) for f, _ in side.get(k, [])}                                     # noqa: E731
    # a copy that REV does not have as well is an error whether or not the bodies agree: two files would have to change together
    twice = sorted(k for k in new if len(new[k]) > 1 and len(new[k]) != len(old.get(k, [])))
    lists = {"differs": sorted(k for k in new if k in old and k not in twice and texts(new[k]) != texts(old[k])),
             "new": sorted(set(new) - set(old)), "gone": sorted(set(old) - set(new)), "defined twice": twice}
    for name in sorted(set(units["old"]) | set(units["new"])):
        mine = {tag: [k for k in ks if name in files(k)] for tag, ks in lists.items()}
        moved = sum(1 for k in units["new"].get(name, {}) if k in old and name not in {f for f, _ in old[k]})
        verdict = "same" if not any(mine.values()) else ", ".join(f"{len(v)} {k}" for k, v in mine.items() if v)
        verdict += f" ({moved} from other files)" if moved else ""
        print(f"{name:22s} {len(units['old'].get(name, {})):4d} -> {len(units['new'].get(name, {})):4d} kernels  {verdict}")
    count = lambda side: sum(len(v) for v in side.values())                                                     # noqa: E731
    print(f"{'all files':22s} {count(old):4d} -> {count(new):4d} kernels  " +
          ("same" if not any(lists.values()) else ", ".join(f"{len(v)} {k}" for k, v in lists.items() if v)))
    for tag, ks in lists.items():
        for k in ks:
            print(f"    {tag}: {k}  [{', '.join(sorted(f for f, _ in new.get(k, old.get(k))))}]")
    return 1 if lists["differs"] or lists["new"] or lists["defined twice"] else 0


if __name__ == "__main__":
    sys.exit(main())

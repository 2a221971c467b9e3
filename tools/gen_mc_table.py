"""Derive the marching-cubes case table from its rule and write cips_3dplusplus_amd/csrc/mc_table.h.

    python tools/gen_mc_table.py [--check]      (--check: compare with the committed header, write nothing)

Conventions (include/cips3d_hip.h, cips3d_marching_cubes_*):
  corner c = x + 2y + 4z of the unit cell, x <-> volume column j, y <-> row i, z <-> depth k;
  edge e of axis a = e // 4 joins its lower corner to lower + e_a; the lower corner of
    x-edges (e 0..3)  is (0, e & 1, e >> 1),
    y-edges (e 4..7)  is ((e - 4) & 1, 0, (e - 4) >> 1),
    z-edges (e 8..11) is ((e - 8) & 1, (e - 8) >> 1, 0);
  case bit c is set when corner c is inside (value < level).

The rule, per case:
  1. on each of the six cube faces, pair the face's crossing edges into segments: two crossings form one segment; on a
     face whose corners form a checkerboard (four crossings) each inside corner is cut off by its own segment, so the
     inside corners are always separated -- a face is resolved from its own four corners alone, and the two cells that
     share it agree;
  2. orient each segment so that, seen from outside the cube, the inside corner region lies on its right;
  3. chain the directed segments into cycles (each crossing edge lies on exactly two faces: one segment enters it and
     one leaves it);
  4. fan-triangulate each cycle from the first of its vertices (smallest edge first) whose diagonals join no two edges
     of one common face: such a diagonal would also be drawn by the neighbouring cell.
Cycles are ordered by their smallest edge; each cycle starts at its smallest edge.  The triangles then wind so that
(v1 - v0) x (v2 - v0) points from the inside corners to the outside ones.
"""
import argparse
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "cips_3dplusplus_amd", "csrc", "mc_table.h")


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_corners(e):
    """(lower corner, upper corner, axis) of cube edge e."""
    a, r = divmod(e, 4)
    lo = [(0, r & 1, r >> 1), (r & 1, 0, r >> 1), (r & 1, r >> 1, 0)][a]
    c0 = lo[0] + 2 * lo[1] + 4 * lo[2]
    return c0, c0 + (1 << a), a


EDGES = [edge_corners(e) for e in range(12)]
EDGE_OF = {frozenset((c0, c1)): e for e, (c0, c1, _) in enumerate(EDGES)}


def faces():
    """Six faces: (outward normal, corners in cyclic order, edges between consecutive corners)."""
    out = []
    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        for s in (0, 1):
            n = np.zeros(3)
            n[ax] = 2 * s - 1
            ring = []
            for pu, pv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[ax], p[u], p[v] = s, pu, pv
                ring.append(p[0] + 2 * p[1] + 4 * p[2])
            edges = [EDGE_OF[frozenset((ring[q], ring[(q + 1) % 4]))] for q in range(4)]
            out.append((n, ring, edges))
    return out


FACES = faces()


def mid(e):
    c0, c1, _ = EDGES[e]
    return 0.5 * (corner_pos(c0) + corner_pos(c1))


def inside_corner(case, e):
    c0, c1, _ = EDGES[e]
    return c0 if case >> c0 & 1 else c1


def face_segments(case):
    """Directed segments (p, q) of every face, inside region on the right seen from outside."""
    segs = []
    for n, ring, edges in FACES:
        ins = [case >> c & 1 for c in ring]
        cross = [e for q, e in enumerate(edges) if ins[q] != ins[(q + 1) % 4]]
        if not cross:
            continue
        if len(cross) == 2:
            pairs = [tuple(cross)]
        else:                                       # checkerboard: cut off each inside corner on its own
            pairs = []
            for q in range(4):
                if ins[q]:
                    pairs.append((edges[(q + 3) % 4], edges[q]))     # the two face edges that meet at ring[q]
        for p, q in pairs:
            ci = corner_pos(inside_corner(case, p))
            side = np.dot(np.cross(n, mid(q) - mid(p)), ci - mid(p))
            assert side != 0
            segs.append((p, q) if side < 0 else (q, p))
    return segs


def share_face(e1, e2):
    return any(e1 in edges and e2 in edges for _, _, edges in FACES)


def cycles(case):
    nxt = {}
    for p, q in face_segments(case):
        assert p not in nxt, (case, "two segments leave one edge")
        nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values()), (case, "segments do not close")
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        cyc, e = [], start
        while e not in seen:
            seen.add(e)
            cyc.append(e)
            e = nxt[e]
        assert e == start
        out.append(cyc)
    return out


def triangulate(cyc):
    n = len(cyc)
    for s in range(n):
        rot = cyc[s:] + cyc[:s]
        if all(not share_face(rot[0], rot[k]) for k in range(2, n - 1)):
            return [(rot[0], rot[k], rot[k + 1]) for k in range(1, n - 1)]
    raise AssertionError(f"no fan of {cyc} avoids a face diagonal")


def case_triangles(case):
    tris = []
    for cyc in cycles(case):
        tris += triangulate(cyc)
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


def render(tab):
    width = max(len(t) for t in tab)
    lines = ["/* Generated by tools/gen_mc_table.py from the rule stated there -- do not edit. */",
             "#pragma once", "",
             "/* triangles per case (case bit c = corner c inside, corner c = x + 2y + 4z) */",
             f"#define MC_MAX_TRIS {width}",
             "#define MC_TRI_COUNT_INIT { \\"]
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join(str(len(t)) for t in tab[r:r + 32]) + ", \\")
    lines.append("}")
    lines.append("/* cube edges of each triangle, MC_MAX_TRIS x 3 per case, -1 past the case's count */")
    lines.append("#define MC_TRI_EDGES_INIT { \\")
    for c, t in enumerate(tab):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (width - len(t)))
        lines.append("  {" + ", ".join(str(e) for e in flat) + "}, \\")
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    text = render(table())
    if args.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_table.h up to date" if same else "mc_table.h differs from the rule")
        raise SystemExit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)


if __name__ == "__main__":
    main()

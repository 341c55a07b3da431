"""Marching-cubes case table, derived from one face rule rather than typed in (mesh export).

Cube corners are numbered c = x + 2 y + 4 z (bit a of c = the corner's offset along axis a).  Cube edge e runs along
axis a = e >> 2 from its base corner, whose two other coordinates are (e & 1, e >> 1 & 1) in increasing axis order, to the
base corner + 1 along a.  A case is the 8-bit mask of the inside corners (value > L).

The rule, per cube face:
  * the crossing edges of a face (its end corners disagree) are joined into segments: two crossing edges -> one segment;
    four (the face's two inside corners are diagonal: ambiguous) -> one segment around each inside corner, which keeps the
    inside corners apart;
  * each segment is directed so that, walking along it with the face's outward normal n, the outside lies on the side of
    n x direction: the loops it closes into then wind counter-clockwise seen from outside (normals toward lower density);
  * the directed segments of the 6 faces close into one or more loops per case; each loop is fan-triangulated from its
    lowest-numbered cube edge.

The segments of a face depend on its four corner signs only, so the two cells that share a face leave the same segments
on it (in opposite directions): the mesh has no cracks.

    python vox-e_amd/voxe_hip/mc_table.py            # rewrite vox-e_amd/csrc/voxe_mc_table.hpp
    python vox-e_amd/voxe_hip/mc_table.py --check    # exit 1 if the committed header differs
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "csrc", "voxe_mc_table.hpp")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_axis(e):
    return e >> 2


def edge_corners(e):
    """(base corner, far corner) of cube edge e"""
    a, o = e >> 2, e & 3
    others = [b for b in range(3) if b != a]
    c0 = ((o & 1) << others[0]) | (((o >> 1) & 1) << others[1])
    return c0, c0 | (1 << a)


def edge_mid(e):
    c0, c1 = edge_corners(e)
    return tuple(0.5 * (p + q) for p, q in zip(corner_pos(c0), corner_pos(c1)))


FACES = [(a, s) for a in range(3) for s in (0, 1)]   # face (a, s): the corners with bit a == s; outward normal (2 s - 1) e_a


def face_corners(face):
    a, s = face
    return [c for c in range(8) if ((c >> a) & 1) == s]


def face_edges(face):
    a, s = face
    return [e for e in range(12) if edge_axis(e) != a and ((edge_corners(e)[0] >> a) & 1) == s]


def face_normal(face):
    a, s = face
    n = [0.0, 0.0, 0.0]
    n[a] = 1.0 if s else -1.0
    return n


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(u, v):
    return tuple(p - q for p, q in zip(u, v))


def _dot(u, v):
    return sum(p * q for p, q in zip(u, v))


def crossing(case, e):
    c0, c1 = edge_corners(e)
    return ((case >> c0) & 1) != ((case >> c1) & 1)


def face_segments(case, face):
    """directed segments (edge_from, edge_to) the rule puts on `face` for the corner signs of `case`"""
    inside = [c for c in face_corners(face) if (case >> c) & 1]
    outside = [c for c in face_corners(face) if not (case >> c) & 1]
    cross = [e for e in face_edges(face) if crossing(case, e)]
    if not cross:
        return []
    n = face_normal(face)
    groups = []   # (edge pair, point on the inside side, point on the outside side)
    if len(cross) == 2:
        cen = lambda cs: tuple(sum(corner_pos(c)[i] for c in cs) / len(cs) for i in range(3))  # noqa: E731
        groups.append((cross, cen(inside), cen(outside)))
    else:   # ambiguous: the two inside corners are diagonal; cut each one off on its own
        for c in inside:
            pair = [e for e in cross if c in edge_corners(e)]
            mid = tuple(0.5 * (p + q) for p, q in zip(edge_mid(pair[0]), edge_mid(pair[1])))
            groups.append((pair, corner_pos(c), mid))
    segs = []
    for (ea, eb), p_in, p_out in groups:
        m = _sub(p_out, p_in)
        d = _sub(edge_mid(eb), edge_mid(ea))
        segs.append((ea, eb) if _dot(d, _cross(m, n)) > 0 else (eb, ea))
    return segs


def case_loops(case):
    """the closed loops (lists of cube edges, each starting at its lowest edge) of `case`"""
    nxt = {}
    for face in FACES:
        for a, b in face_segments(case, face):
            assert a not in nxt, (case, face, a)
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)   # starts at its smallest edge: `start` is the smallest unseen edge
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def table():
    """[256] lists of (e0, e1, e2) cube-edge triangles"""
    return [case_triangles(c) for c in range(256)]


def header_text():
    tab = table()
    K = max(len(t) for t in tab)
    lines = [
        "// voxe_mc_table.hpp -- GENERATED by vox-e_amd/voxe_hip/mc_table.py; do not edit.",
        "// Marching-cubes case table: case = bit c set when cube corner c (= x + 2 y + 4 z) is inside; triangles are triples of",
        "// cube edges e (axis e >> 2, base corner offsets (e & 1, e >> 1 & 1) along the two other axes in increasing order),",
        "// wound counter-clockwise seen from outside.  Unused slots hold 0xff.",
        "#pragma once",
        "",
        f"#define VOXE_MC_MAX_TRIS {K}",
        "",
        "__constant__ unsigned char kMcTriCount[256] = {",
    ]
    counts = [len(t) for t in tab]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(c) for c in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"__constant__ unsigned char kMcTriEdges[256][{3 * K}] = {{")
    for c, tris in enumerate(tab):
        flat = [e for t in tris for e in t] + [255] * (3 * (K - len(tris)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + f"}},  // {c}")
    lines.append("};")
    lines.append("")
    lines.append("// base corner of cube edge e: the lattice node that owns the edge's vertex is the cell's min node + this corner")
    lines.append("__constant__ unsigned char kMcEdgeBase[12] = {" + ", ".join(str(edge_corners(e)[0]) for e in range(12)) + "};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = header_text()
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("up to date" if same else f"{HEADER} differs from the generator's output")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

"""What can be known of iso-surface extraction without a GPU: the generated case table (``csrc/ag_isosurface_table.h``) against the oracle's
own restatement of the rule and against the rule's properties, the oracle's meshes on closed fields, and the ABI's declarations.
Every test prints its own figures."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isosurface_oracle as io  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "animatablegaussians_amd", "csrc")
HEADER = os.path.join(CSRC, "ag_isosurface_table.h")


def _parse_header(path):
    text = open(path).read()
    code = re.sub(r"//[^\n]*", "", text)
    count = re.search(r"kIsoTriCount\[256\]\s*=\s*\{([^}]*)\}", code).group(1)
    count = np.array([int(x) for x in count.replace("\n", " ").split(",") if x.strip()])
    body = code[code.index("kIsoTriTable"):]
    rows = re.findall(r"\{([-\d,\s]+)\}", body[body.index("=") + 1:])
    table = np.array([[int(x) for x in r.split(",")] for r in rows])
    return table, count


def test_header_equals_the_oracles_table():
    table, count = _parse_header(HEADER)
    assert table.shape == (256, 16) and count.shape == (256,)
    for case in range(256):
        assert np.array_equal(table[case], io.TRI_TABLE[case]), f"case {case}: header {table[case]} / oracle {io.TRI_TABLE[case]}"
    assert np.array_equal(count, io.TRI_COUNT)
    print(f"256 rows equal; {int(count.sum())} triangles")


def test_generator_reproduces_the_committed_header(tmp_path):
    out = str(tmp_path / "table.h")
    subprocess.check_call([sys.executable, os.path.join(CSRC, "gen_isosurface_table.py"), out])
    assert open(out, "rb").read() == open(HEADER, "rb").read(), "ag_isosurface_table.h is not what gen_isosurface_table.py writes"


def _crossed_edges(case):
    out = set()
    for e in range(12):
        lo, hi = io._edge_corners(e)
        if ((case >> io._cid(lo)) & 1) != ((case >> io._cid(hi)) & 1):
            out.add(e)
    return out


def test_table_properties_for_all_cases():
    table, count = _parse_header(HEADER)
    for case in range(256):
        tris = table[case][table[case] >= 0].reshape(-1, 3)
        assert len(tris) == count[case] <= 5 and (table[case][3 * len(tris):] == -1).all()
        crossed = _crossed_edges(case)
        assert set(tris.reshape(-1).tolist()) == crossed, f"case {case}: the triangles use {set(tris.reshape(-1).tolist())}, crossed {crossed}"
        half = {}
        for a, b, c in tris.tolist():
            assert len({a, b, c}) == 3
            for h in ((a, b), (b, c), (c, a)):
                assert h not in half, f"case {case}: half-edge {h} twice"
                half[h] = 1
        boundary = {h for h in half if (h[1], h[0]) not in half}
        interior = {h for h in half if (h[1], h[0]) in half}
        # the triangles are the loops reversed, so a boundary half-edge (a, b) is the rule's segment b -> a of the face it lies in
        want = set()
        for walk in io.FACE_WALKS:
            for a, b in io.face_segments(walk, case):
                want.add((b, a))
        assert boundary == want, f"case {case}: half-edges used once {sorted(boundary)}, the rule's segments reversed {sorted(want)}"
        for a, b in boundary:
            assert io._share_face(a, b)
        for a, b in interior:
            assert not io._share_face(a, b), f"case {case}: the interior diagonal {a}-{b} joins two cube edges of a common face"
    loops = sum(len(_loops(case)) for case in range(256))
    print(f"256 cases: {int(count.sum())} triangles, at most {int(count.max())} per case, {loops} polygons")
    assert int(count.sum()) == 820 and loops == 358


def _loops(case):
    follow = {}
    for walk in io.FACE_WALKS:
        follow.update(dict(io.face_segments(walk, case)))
    loops, seen = [], set()
    for e in sorted(follow):
        if e in seen:
            continue
        loop = []
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = follow[e]
        loops.append(loop)
    return loops


def test_face_rule_reads_only_the_faces_bits_and_joins_inside_corners():
    """Two cells that share a face see the same four bits, so equal segments up to direction: checked by flipping every bit that is not
    on the face.  On the ambiguous face each segment cuts off one OUTSIDE corner (the inside corners stay joined)."""
    for walk in io.FACE_WALKS:
        on_face = sum(1 << io._cid(p) for p in walk)
        for case in range(256):
            assert io.face_segments(walk, case) == io.face_segments(walk, case & on_face) == io.face_segments(walk, case | (255 & ~on_face))
        amb = (1 << io._cid(walk[0])) | (1 << io._cid(walk[2]))                     # inside: corners 0 and 2 of the walk
        for a, b in io.face_segments(walk, amb):
            shared = set(io._edge_corners(a)) & set(io._edge_corners(b))
            assert len(shared) == 1 and not (amb >> io._cid(next(iter(shared)))) & 1


def test_noise_fields_are_closed_and_oriented():
    for seed in range(4):
        vol = io.noise_field((8, 7, 9), seed, closed=True)
        v, f = io.extract(vol, 0.0, dtype=np.float64)
        keys, counts, closed = io.directed_edge_census(f)
        print(f"seed {seed}: V {len(v)}, F {len(f)}, directed edges {len(keys)}, most often {int(counts.max())}, Euler {io.euler_characteristics(f, len(v))}")
        assert len(f) > 500 and closed and len(keys) == 3 * len(f)


def test_sphere_and_torus():
    for name, vol, chi, exact in (("sphere", io.sphere_field((14, 14, 14), (6.3, 6.6, 6.4), 4.2), 2, 4 / 3 * np.pi * 4.2 ** 3),
                                  ("torus", io.torus_field((14, 14, 14), (6.4, 6.6, 6.5), 4.0, 1.6), 0, 2 * np.pi ** 2 * 4.0 * 1.6 ** 2)):
        v, f = io.extract(vol, 0.0, dtype=np.float64)
        vol_signed = io.signed_volume(v, f)
        print(f"{name}: V {len(v)}, F {len(f)}, Euler {io.euler_characteristics(f, len(v))}, signed volume {vol_signed:.3f} (the smooth body's {exact:.3f})")
        assert io.directed_edge_census(f)[2] and io.euler_characteristics(f, len(v)) == [chi]
        assert 0.8 * exact < vol_signed < exact            # positive: wound counter-clockwise seen from outside; chords lie inside a convex body


def test_float32_and_float64_oracles_share_the_faces():
    sp, org = (0.03, 0.02, 0.01), (-0.4, 1.1, 0.05)
    vol = io.noise_field((9, 8, 7), 2)
    v32, f32 = io.extract(vol, 0.137, sp, org, None, np.float32)
    v64, f64 = io.extract(vol, 0.137, sp, org, None, np.float64)
    assert v32.dtype == np.float32 and np.array_equal(f32, f64) and f32.dtype == np.int32
    dev = float(np.abs(v32.astype(np.float64) - v64).max())
    print(f"V {len(v32)}, F {len(f32)}, |float32 - float64| oracle {dev:.3e}")
    assert dev < 1e-6


def _declarations():
    hdr = open(os.path.join(ROOT, "include", "ag_isosurface.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(ag_isosurface_[a-z_]+)\s*\(([^)]*)\)", hdr):
        out[name] = (ret, [" ".join(a.split()[:-1]) for a in args.split(",")])
    return out


def test_abi_symbols_match_the_header():
    from animatablegaussians_amd import _lib
    ctype = {"int32_t": _lib.c_i32, "float": _lib.c_f, "size_t": _lib.c_sz, "const float*": _lib.c_vp, "const uint8_t*": _lib.c_vp, "void*": _lib.c_vp,
             "const void*": _lib.c_vp, "float*": _lib.c_vp, "int32_t*": _lib.c_vp, "int": ctypes.c_int}
    host = {"ag_isosurface_emit": {5: ctypes.POINTER(_lib.c_f), 6: ctypes.POINTER(_lib.c_f)}}          # spacing, origin: HOST [3]
    decl = _declarations()
    assert set(decl) == {"ag_isosurface_workspace_bytes", "ag_isosurface_count", "ag_isosurface_emit"}
    table = {s[0]: s for s in _lib.SYMBOLS}
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in decl.items():
        assert name in table and hasattr(L, name), name
        want = [host.get(name, {}).get(i, ctype[a]) for i, a in enumerate(args)]
        assert table[name][1] is ctype[ret] and table[name][2] == want, f"{name}: binding {table[name][2]} / header {args}"
        print(name, len(args), "arguments")
    # the sizes-only refusals need no GPU
    L.ag_isosurface_workspace_bytes.restype = ctypes.c_size_t
    assert L.ag_isosurface_workspace_bytes(1, 4, 4) == 0 and L.ag_isosurface_workspace_bytes(1024, 1024, 1024) == 0
    n = L.ag_isosurface_workspace_bytes(256, 256, 128)
    print(f"workspace at (256, 256, 128): {n} bytes")
    assert 17 * 256 * 256 * 128 <= n <= 18 * 256 * 256 * 128


def test_every_case_volume_carries_every_case():
    vol, mask = io.every_case_volume()
    inside = vol >= 0
    for c, corner in itertools.product(range(256), range(8)):
        assert inside[corner & 1, (corner >> 1) & 1, 3 * c + (corner >> 2)] == bool((c >> corner) & 1)
    v, f = io.extract(vol, 0.0, mask=mask)
    assert len(f) == 820 and (np.abs(vol) >= 0.25).all() and (np.abs(vol) <= 1).all()

"""The scene tables of acn_scene_upload (actinon_amd/csrc/acn_tables.cpp) on the CPU: the GNode / GMat split with its pair and
prune-level flags, the cost-ordered element copy, the interval-prune programs, the simple-compound pre-order tables and the LDS
plan.  Three kinds of check:
  - digests: every table is byte-identical to what the commit before this unit existed built inside acn_scene_upload, recorded
    once from that commit for every scene and option arm below (tests/golden/upload_tables.json);
  - structure: an independent numpy walk over the tables -- a wrong skip link or an overdeep prune program is an out-of-bounds
    read or an LDS overrun on the device, so it has to show here first;
  - validation: every message of acn_tables_validate, from a flat scene with one field broken."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import actinon_amd as A
from actinon_amd import abi
import scenes_util as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SCENES = ["primitives", "wine_glass", "diamond", "many_spheres:3:1", "many_spheres:4:1", "textured",
          "hanging_lamp", "paraffin_lamp_on_ledge", "hanging_lamps_in_row"]
# arm -> (switches: no_leaf_pairs, no_pair2, no_prune_levels, no_simple_compounds, no_sc_cull, no_sc_reversed; prune_min; lds_max)
ARMS = {
    "default":             ((0, 0, 0, 0, 0, 0), -1, -1),
    "prune_min_1":         ((0, 0, 0, 0, 0, 0), 1, -1),       # ACN_PRUNE_MIN=1
    "no_sc_cull":          ((0, 0, 0, 0, 1, 0), -1, -1),      # ACN_NO_SC_CULL=1
    "no_sc_reversed":      ((0, 0, 0, 0, 0, 1), -1, -1),      # ACN_NO_SC_REVERSED=1
    "no_prune_levels":     ((0, 0, 1, 0, 0, 0), -1, -1),      # ACN_NO_PRUNE_LEVELS=1
    "no_leaf_pairs":       ((1, 0, 0, 0, 0, 0), -1, -1),      # ACN_NO_LEAF_PAIRS=1
    "no_pair2":            ((0, 1, 0, 0, 0, 0), -1, -1),      # ACN_NO_PAIR2=1
    "no_simple_compounds": ((0, 0, 0, 1, 0, 0), -1, -1),      # ACN_NO_SIMPLE_COMPOUNDS=1
    "lds_max_0":           ((0, 0, 0, 0, 0, 0), -1, 0),       # ACN_LDS_MAX=0
}
CASES = [(s, a) for s in SCENES for a in ARMS]

TABLES = ["nodes", "mats", "elems", "sc_table", "sc_spheres"]
GNODE = np.dtype([("type", "<i4"), ("flags", "<u4"), ("child0", "<i4"), ("child1", "<i4"), ("prm", "<f8", 4), ("pos", "<f8", 3),
                  ("env_pos", "<f8", 3), ("env_radius", "<f8"), ("rax", "<f8", 9), ("surface_roughness", "<f8"),
                  ("sdf_kind", "<i4"), ("cycles", "<i4")])
GMAT = np.dtype([("color", "<f8", 3), ("radiance", "<f8"), ("refractive_index", "<f8"), ("fresnel_reflectivity", "<f8"),
                 ("chromatic_reflectivity", "<f8"), ("diffuse_reflectivity", "<f8"), ("sigma", "<f8"), ("transparency", "<f8", 3),
                 ("texture", "<i4"), ("pad_", "<i4")])
SCENTRY = np.dtype([("env_pos", "<f8", 3), ("env_radius", "<f8"), ("node", "<i4"), ("skip", "<i4"), ("type", "<i4"), ("flags", "<u4")])
DTYPES = {"nodes": GNODE, "mats": GMAT, "elems": np.dtype("<i4"), "sc_table": SCENTRY, "sc_spheres": np.dtype("<f8")}
assert (GNODE.itemsize, GMAT.itemsize, SCENTRY.itemsize) == (192, 104, 48)

# acn_tables.h
SC_SPHERE, SC_ROUGH, SC_BOUNDING = 0x10000, 0x20000, 0x40000
GFLAG_SIMPLE_COMPOUND, GFLAG_PRUNE_LEVELS_SHIFT = 0x200, 12
PO_END, PO_PLANE, PO_SPHERE, PO_QUAD, PO_ALL, PO_NEG, PO_AND, PO_OR, PO_ENV = range(9)
PRUNE_STACK, PRUNE_MAX_OPS = 5, 256
SCALARS = ["prune_base", "elem_pos_base", "prune", "leaf_lights", "n_lights", "n_levels", "lds_bytes", "lds_stack_bytes"]


@pytest.fixture(scope="module")
def lib():
    srcs = [os.path.join(HERE, "csrc", "tables_cpu.cpp"), os.path.join(ROOT, "actinon_amd", "csrc", "acn_tables.cpp")]
    deps = srcs + [os.path.join(ROOT, "actinon_amd", "csrc", "acn_tables.h"), os.path.join(ROOT, "include", "actinon_hip.h")]
    out = os.path.join(ROOT, "build", "libtables_cpu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "actinon_amd", "csrc")] + srcs + ["-o", out])
    l = C.CDLL(out)
    l.tables_build.argtypes = [C.POINTER(abi.FlatScene), C.POINTER(C.c_int), C.c_longlong, C.c_longlong]
    l.tables_build.restype = C.c_void_p
    l.tables_bytes.argtypes = [C.c_void_p, C.c_int]
    l.tables_bytes.restype = C.c_size_t
    l.tables_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    l.tables_scalars.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    l.tables_free.argtypes = [C.c_void_p]
    l.tables_validate.argtypes = [C.POINTER(abi.FlatScene), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    return l


def flatten(name):
    if name == "textured":
        return S.build_textured().flatten()
    if name in A.Scene.BUILDERS or name.startswith("many_spheres"):
        return A.Scene.build(name).flatten()
    return A.Flat.load(os.path.join(HERE, "golden", "scenes", name + ".npz"))


class Built:
    """The tables of one scene under one option arm: raw bytes, numpy views, scalars, and the flat scene they came from."""

    def __init__(self, lib, flat, arm):
        switches, prune_min, lds_max = ARMS[arm]
        t = lib.tables_build(C.byref(flat.c), (C.c_int * 6)(*switches), prune_min, lds_max)
        self.raw = {}
        for k, name in enumerate(TABLES):
            buf = C.create_string_buffer(max(1, lib.tables_bytes(t, k)))
            lib.tables_copy(t, k, buf)
            self.raw[name] = buf.raw[:lib.tables_bytes(t, k)]
        sc = (C.c_ulonglong * 8)()
        lib.tables_scalars(t, sc)
        lib.tables_free(t)
        self.scalars = dict(zip(SCALARS, (int(v) for v in sc)))
        for name in TABLES:
            setattr(self, name, np.frombuffer(self.raw[name], dtype=DTYPES[name]))
        self.flat = flat
        self.n_nodes, self.n_elems = flat.c.n_nodes, flat.c.n_elems
        self.in_nodes = np.frombuffer(flat.nodes_bytes(), dtype=np.dtype(abi.Node))
        self.in_elems = np.ctypeslib.as_array(flat.c.elems, shape=(max(1, self.n_elems),))[:self.n_elems].copy()
        self.offsets = self.elems[self.scalars["prune_base"]:self.scalars["prune_base"] + self.n_nodes]


@pytest.fixture(scope="module")
def built(lib):
    flats, cache = {}, {}

    def get(scene, arm):
        if scene not in flats:
            flats[scene] = flatten(scene)
        if (scene, arm) not in cache:
            cache[scene, arm] = Built(lib, flats[scene], arm)
        return cache[scene, arm]
    return get


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "upload_tables.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------
# 1. digests

@pytest.mark.parametrize("scene,arm", CASES)
def test_tables_are_byte_identical_to_the_recorded_upload(built, golden, lib, scene, arm):
    b, want = built(scene, arm), golden[scene][arm]
    for name in TABLES:
        got = {"sha256": hashlib.sha256(b.raw[name]).hexdigest(), "len": len(b.raw[name]) // DTYPES[name].itemsize}
        assert got == want["tables"][name], f"{scene} / {arm}: table '{name}' differs from the recorded one"
    for k in SCALARS:
        assert b.scalars[k] == want["scalars"][k], f"{scene} / {arm}: {k}"
    max_csg, err = C.c_int(-1), C.create_string_buffer(256)
    assert lib.tables_validate(C.byref(b.flat.c), C.byref(max_csg), err, 256) == abi.ACN_OK and err.value == b""
    assert max_csg.value == want["scalars"]["max_csg"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. structure

@pytest.mark.parametrize("scene,arm", CASES)
def test_cost_order_is_a_permutation_with_its_positions(built, scene, arm):
    b = built(scene, arm)
    n, base = b.n_elems, b.scalars["elem_pos_base"]
    assert b.scalars["prune_base"] == 2 * n and base + n + 1 == len(b.elems)
    assert np.array_equal(b.elems[:n], b.in_elems)
    ordered, elem_pos = b.elems[n:2 * n], b.elems[base:base + n]
    for i in np.flatnonzero(b.in_nodes["type"] == abi.ACN_COMPOUND):
        c0, c1 = int(b.in_nodes["child0"][i]), int(b.in_nodes["child1"][i])
        assert np.array_equal(np.sort(ordered[c0:c0 + c1]), np.sort(b.in_elems[c0:c0 + c1])), f"compound {i}"
        pos = elem_pos[c0:c0 + c1]
        assert ((pos >= 0) & (pos < max(c1, 1))).all(), f"compound {i}"
        assert np.array_equal(ordered[c0:c0 + c1], b.elems[c0 + pos]), f"compound {i}"


def is_pair(t):
    return t in (abi.ACN_PAIR_INSIDE, abi.ACN_PAIR_OUTSIDE)


@pytest.mark.parametrize("scene,arm", CASES)
def test_prune_programs_stay_within_their_budgets(built, scene, arm):
    b = built(scene, arm)
    types, flags = b.in_nodes["type"], b.in_nodes["flags"]
    assert ((b.offsets == -1) | ((b.offsets >= b.scalars["prune_base"] + b.n_nodes) & (b.offsets < len(b.elems)))).all()
    leaf_type = {PO_PLANE: abi.ACN_PLANE, PO_SPHERE: abi.ACN_SPHERE, PO_QUAD: abi.ACN_SQUAROID}
    programs = 0
    for node in np.flatnonzero(b.offsets >= 0):
        if not is_pair(types[node]):
            assert types[node] == abi.ACN_COMPOUND and b.nodes["flags"][node] & GFLAG_SIMPLE_COMPOUND   # a simple compound's header
            continue
        programs += 1
        pc, depth, ended = int(b.offsets[node]), 0, False
        for _ in range(PRUNE_MAX_OPS):
            assert pc < b.scalars["elem_pos_base"], f"program of node {node} runs out of its area"
            w = int(b.elems[pc]) & 0xFFFFFFFF
            op, arg = w & 15, w >> 4
            pc += 1
            assert op <= PO_ENV and arg < b.n_nodes
            if op == PO_END:
                ended = True
                break
            if op <= PO_ALL:
                depth += 1
                assert depth <= PRUNE_STACK, f"program of node {node}: interval stack overflows"
                assert arg == 0 if op == PO_ALL else types[arg] == leaf_type[op]
            elif op == PO_NEG:
                assert depth >= 1 and (arg == 0 or (types[arg] == abi.ACN_PLANE and not flags[arg] & abi.ACN_NODE_HAS_ENVELOPE))
            elif op == PO_ENV:
                assert depth >= 1 and flags[arg] & abi.ACN_NODE_HAS_ENVELOPE
            else:
                assert depth >= 2 and arg == 0, f"program of node {node}: interval stack underflows"
                depth -= 1
        assert ended, f"program of node {node} has no END within {PRUNE_MAX_OPS} ops"
        assert depth == 1, f"program of node {node} leaves {depth} intervals"
    if arm == "prune_min_1":
        roots = {int(e) for i in np.flatnonzero(types == abi.ACN_COMPOUND)
                 for e in b.in_elems[b.in_nodes["child0"][i]:b.in_nodes["child0"][i] + b.in_nodes["child1"][i]] if is_pair(types[e])}
        assert programs == len(roots)   # every CSG root element of every compound has one
    assert bool(b.scalars["prune"]) == bool((b.offsets >= 0).any())


def walk_preorder(b, lo, hi, compound, reverse):
    """Entries [ lo, hi ) are the children of `compound`, each compound child followed by its own subtree: checks links and order."""
    c0, c1 = int(b.in_nodes["child0"][compound]), int(b.in_nodes["child1"][compound])
    want = list(b.in_elems[c0:c0 + c1])
    if reverse:
        want.reverse()
    seen, i = [], lo
    while i < hi:
        e = b.sc_table[i]
        node = int(e["node"])
        seen.append(node)
        assert 0 <= node < b.n_nodes and e["type"] == b.in_nodes["type"][node]
        assert np.array_equal(e["env_pos"], b.in_nodes["env_pos"][node]) and e["env_radius"] == b.in_nodes["env_radius"][node]
        assert (int(e["flags"]) & 1) == (int(b.in_nodes["flags"][node]) & abi.ACN_NODE_HAS_ENVELOPE)
        if e["type"] == abi.ACN_COMPOUND:
            skip = int(e["skip"])
            assert i < skip <= hi, f"entry {i}: skip {skip} outside ( {i}, {hi} ]"
            walk_preorder(b, i + 1, skip, node, reverse)
            i = skip
        else:
            sphere = e["type"] == abi.ACN_SPHERE
            assert bool(e["flags"] & SC_SPHERE) == sphere
            if sphere:   # the link of a sphere leaf names its record
                rec = b.sc_spheres[4 * int(e["skip"]):4 * int(e["skip"]) + 4]
                assert len(rec) == 4 and np.array_equal(rec[:3], b.in_nodes["pos"][node]) and rec[3] == b.in_nodes["prm"][node][0]
                assert bool(e["flags"] & SC_ROUGH) == bool(b.in_nodes["surface_roughness"][node] > 0)
            else:
                assert e["type"] in (abi.ACN_PLANE, abi.ACN_SQUAROID) and int(e["skip"]) == i + 1
            i += 1
    assert seen == want, f"children of compound {compound}"


def check_bounding(b, lo, hi):
    """Every ACN_SC_BOUNDING entry of [ lo, hi ) contains all leaves below it, by the builder's own inequality."""
    t = b.sc_table
    for i in lo + np.flatnonzero(t["flags"][lo:hi] & SC_BOUNDING):
        end = int(t["skip"][i]) if t["type"][i] == abi.ACN_COMPOUND else i + 1
        below = t[i:end]
        leaves = below["node"][below["type"] != abi.ACN_COMPOUND]
        assert (b.in_nodes["type"][leaves] == abi.ACN_SPHERE).all()
        d = b.in_nodes["pos"][leaves] - t["env_pos"][i]
        d2 = (0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        assert (np.sqrt(d2) + np.abs(b.in_nodes["prm"][leaves][:, 0]) <= abs(t["env_radius"][i]) * (1.0 - 1E-9)).all(), f"entry {i}"


@pytest.mark.parametrize("scene,arm", CASES)
def test_simple_compound_tables_link_and_bound_what_they_say(built, scene, arm):
    b = built(scene, arm)
    marked = np.flatnonzero(b.nodes["flags"] & GFLAG_SIMPLE_COMPOUND)
    if arm == "no_simple_compounds":
        assert len(marked) == 0 and len(b.sc_table) == 0 and len(b.sc_spheres) == 0
    if arm == "no_sc_cull":
        assert not (b.sc_table["flags"] & SC_BOUNDING).any()
    covered = 0
    for node in marked:
        off = int(b.offsets[node])
        assert b.in_nodes["type"][node] == abi.ACN_COMPOUND and off >= 0
        first, count, rev, rev_dir = (int(v) for v in b.elems[off:off + 4])
        assert 0 <= first and first + count <= len(b.sc_table)
        walk_preorder(b, first, first + count, node, False)
        check_bounding(b, first, first + count)
        covered += count
        if rev < 0:
            assert rev == -1 and rev_dir == 0
            continue
        assert arm not in ("no_sc_reversed", "no_sc_cull") and count >= 64 and rev + count <= len(b.sc_table)
        walk_preorder(b, rev, rev + count, node, True)
        check_bounding(b, rev, rev + count)
        fwd, bwd = b.sc_table[first:first + count], b.sc_table[rev:rev + count]
        assert sorted(zip(fwd["node"].tolist(), fwd["flags"].tolist())) == sorted(zip(bwd["node"].tolist(), bwd["flags"].tolist()))
        direction = b.sc_spheres[4 * rev_dir:4 * rev_dir + 4]
        assert len(direction) == 4 and direction[3] == 0.0 and abs(np.sqrt((direction[:3] ** 2).sum()) - 1.0) < 1e-12
        covered += count
    assert covered == len(b.sc_table)
    if scene.startswith("many_spheres") and arm == "default":
        assert len(marked) == 1 and (b.sc_table["flags"] & SC_BOUNDING).any() and int(b.elems[int(b.offsets[marked[0]]) + 2]) > 0


@pytest.mark.parametrize("scene,arm", CASES)
def test_prune_levels_and_lds_plan_are_in_range(built, scene, arm):
    b = built(scene, arm)
    levels = (b.nodes["flags"] >> GFLAG_PRUNE_LEVELS_SHIFT) & 7
    assert (levels <= 4).all()
    if arm == "no_prune_levels":
        assert (levels == 4).all()
    assert b.scalars["lds_bytes"] in (0, 192 * b.n_nodes)
    if b.scalars["lds_bytes"]:
        assert b.scalars["lds_bytes"] + b.scalars["lds_stack_bytes"] <= 40960
    if arm == "lds_max_0":
        assert b.scalars["lds_bytes"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. validation: one case per message, each a flat scene with one field broken

def first_node(flat, pred):
    return next(i for i in range(flat.c.n_nodes) if pred(flat.c.nodes[i]))


def root_elem(flat, root, pred=lambda n: True):
    r = flat.c.nodes[root]
    return next(r.child0 + k for k in range(r.child1) if pred(flat.c.nodes[flat.c.elems[r.child0 + k]]))


def chain(wrapper, depth):
    """light: one sphere; matter: `depth` nested wrappers (ACN_COMPOUND or ACN_NEG) around a sphere."""
    n = depth + 4
    nodes, elems = (abi.Node * n)(), (C.c_int32 * n)()
    for i in range(n):
        nodes[i].type, nodes[i].child0, nodes[i].child1, nodes[i].texture = abi.ACN_SPHERE, -1, -1, -1
    for i, (c0, c1) in enumerate([(0, 1), (1, 1)]):   # nodes 0, 1: the roots; node 2: the light; elems[ k ] = k + 2
        nodes[i].type, nodes[i].child0, nodes[i].child1 = abi.ACN_COMPOUND, c0, c1
    for i in range(n - 2):
        elems[i] = i + 2
    for i in range(3, 3 + depth):   # node i wraps node i + 1
        nodes[i].type = wrapper
        nodes[i].child0, nodes[i].child1 = (i - 1, 1) if wrapper == abi.ACN_COMPOUND else (i + 1, -1)
    f = A.Flat()
    f._keep = (nodes, elems)
    f.c.abi_version, f.c.n_nodes, f.c.n_elems, f.c.light_root, f.c.matter_root = abi.ACN_ABI_VERSION, n, n - 2, 0, 1
    f.c.nodes, f.c.elems = C.cast(nodes, C.POINTER(abi.Node)), C.cast(elems, C.POINTER(C.c_int32))
    f.c.params.image_width, f.c.params.image_height, f.c.params.trace_depth = 4, 4, 10
    return f


def broken(case):
    """-> ( flat scene, code, message )"""
    base = "textured" if "texture" in case else "many_spheres:3:1" if case == "nested_cycle" else "wine_glass" if case in ("pair_child", "bad_neg_child", "csg_cycle") else "primitives"
    f = flatten(base) if case not in ("compounds_too_deep", "csg_too_deep") else None
    c = f.c if f else None
    node = lambda pred: c.nodes[first_node(f, pred)]
    ARG, UNS = abi.ACN_ERR_ARG, abi.ACN_ERR_UNSUPPORTED
    if case == "null_nodes":
        c.nodes = C.POINTER(abi.Node)(); return f, ARG, "null scene"
    if case == "abi_version":
        c.abi_version += 1; return f, ARG, "abi_version mismatch"
    if case == "root_index":
        c.matter_root = c.n_nodes; return f, ARG, "bad root index"
    if case == "null_elems":
        c.elems = C.POINTER(C.c_int32)(); return f, ARG, "null elems"
    if case == "experimental_level":
        c.params.experimental_level = 1; return f, UNS, "Unsupported experimental level"
    if case == "image_size":
        c.params.image_height = 1; return f, ARG, "image size"
    if case == "trace_depth":
        c.params.trace_depth = 61; return f, UNS, "trace_depth exceeds device path-level limit"
    if case == "texture_index":
        node(lambda n: n.texture >= 0).texture = c.n_textures; return f, ARG, "bad texture index"
    if case == "texture_kind":
        c.textures[node(lambda n: n.texture >= 0).texture].kind = 7; return f, ARG, "unknown texture kind"
    if case == "chess_texture_without_projection":
        c.textures[node(lambda n: n.texture >= 0 and n.type == abi.ACN_SQUAROID).texture].kind = 1
        return f, UNS, "object has no projection-function for a chess texture (objects.c:240-245)"
    if case == "sdf_kind":
        node(lambda n: n.type == abi.ACN_DISTANCE).sdf_kind = 9; return f, UNS, "unknown distance function"
    if case == "pair_child":
        node(lambda n: is_pair(n.type)).child1 = -1; return f, ARG, "bad pair child"
    if case == "bad_neg_child":
        node(lambda n: n.type == abi.ACN_NEG).child0 = c.n_nodes; return f, ARG, "bad child"
    if case == "compound_slice":
        c.nodes[c.matter_root].child1 = c.n_elems + 1; return f, ARG, "bad compound slice"
    if case == "element_index":
        c.elems[root_elem(f, c.matter_root)] = -1; return f, ARG, "bad element index"
    if case == "node_type":
        node(lambda n: n.type == abi.ACN_SPHERE).type = 0; return f, ARG, "unknown node type"
    if case == "root_type":
        c.matter_root = first_node(f, lambda n: n.type == abi.ACN_SPHERE); return f, ARG, "roots must be compounds"
    if case == "compound_light":
        c.elems[root_elem(f, c.light_root)] = c.matter_root; return f, ARG, "light elements must be objects (scene.c:547)"
    if case == "light_without_fov":
        c.elems[root_elem(f, c.light_root)] = first_node(f, lambda n: n.type == abi.ACN_SQUAROID)
        return f, abi.ACN_ERR_NO_FOV, "light object has no fov-function (objects.c:254-258)"
    if case == "csg_cycle":
        e = c.elems[root_elem(f, c.matter_root, lambda n: is_pair(n.type))]
        c.nodes[e].child0 = e; return f, ARG, "cyclic node graph"
    if case == "nested_cycle":
        c.elems[root_elem(f, c.matter_root)] = c.matter_root; return f, ARG, "compound nesting too deep / cyclic"
    if case == "compounds_too_deep":
        return chain(abi.ACN_COMPOUND, 12), UNS, "compound nesting exceeds device limit"   # 12 below the root: 13 levels, the limit is 12
    if case == "csg_too_deep":
        return chain(abi.ACN_NEG, 25), UNS, "CSG nesting exceeds device limit"             # the limit is 24
    raise KeyError(case)


VALIDATION = ["null_nodes", "abi_version", "root_index", "null_elems", "experimental_level", "image_size", "trace_depth", "texture_index",
              "texture_kind", "chess_texture_without_projection", "sdf_kind", "pair_child", "bad_neg_child", "compound_slice",
              "element_index", "node_type", "root_type", "compound_light", "light_without_fov", "csg_cycle", "nested_cycle",
              "compounds_too_deep", "csg_too_deep"]


@pytest.mark.parametrize("case", VALIDATION)
def test_validation_refuses_with_the_code_and_text_of_the_upload(lib, case):
    flat, code, text = broken(case)
    max_csg, err = C.c_int(0), C.create_string_buffer(256)
    assert lib.tables_validate(C.byref(flat.c), C.byref(max_csg), err, 256) == code
    assert err.value.decode() == text


def test_the_deepest_chains_the_device_takes_pass_validation(lib):
    for flat, want in ((chain(abi.ACN_COMPOUND, 11), 0), (chain(abi.ACN_NEG, 24), 24)):
        max_csg, err = C.c_int(-1), C.create_string_buffer(256)
        assert lib.tables_validate(C.byref(flat.c), C.byref(max_csg), err, 256) == abi.ACN_OK, err.value
        assert max_csg.value == want

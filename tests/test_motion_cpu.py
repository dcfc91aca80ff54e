"""acn_reproject_moving, acn_motion_from_scenes and actinon_amd.motion.rigid_copy (include/actinon_hip.h) without a GPU: the numpy model
of tests/motion_model.py against reproject_model where every row is REST and against answers written down here, the host library's
table against the model bit for bit, rigid_copy against the host library's own transforms, the two rendered frames of the GPU test
on the oracle's first hits, and csrc/acn_motion_host.h in a stand-alone program built with the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import motion_model as MM
import reproject_model as R
import stats_model as T
import surface_model as F
from actinon_amd import abi
from actinon_amd._lib import hip, host
from actinon_amd.motion import subtree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def plain_raster(n=4.0, seed=1):
    """a previous raster without special pixels: the surface points of the pixel centres, records of n samples"""
    rng = np.random.default_rng(seed)
    surf = np.stack([R.surface_record(x + 0.5, y + 0.5) for y in range(R.PH) for x in range(R.PW)])
    st = np.zeros((R.PW * R.PH, 8))
    st[:, 0] = n
    st[:, 1:4] = rng.uniform(0.0, 2.0, (len(st), 3))
    st[:, 4:7] = rng.uniform(0.0, 1.0, (len(st), 3))
    return surf, st


# ---- the header and the mirror ----
def test_symbols_and_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in ("acn_reproject_moving", "acn_reproject_moving_dev", "acn_motion_from_scenes"):
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert hasattr(hip, name)
    for method in ("reproject_moving", "reproject_moving_dev"):
        assert callable(getattr(A.Handle, method))
    assert callable(A.motion_from_scenes) and callable(A.rigid_copy)
    define = lambda name: re.search(r"^#define " + name + r"\s+(.+?)\s*(/\*.*)?$", text, re.M).group(1)
    assert int(define("ACN_MOTION_STRIDE")) == abi.ACN_MOTION_STRIDE == MM.STRIDE == 16
    assert float(define("ACN_MOTION_REST")) == abi.ACN_MOTION_REST == MM.REST == 0.0
    assert float(define("ACN_MOTION_MOVED")) == abi.ACN_MOTION_MOVED == MM.MOVED == 1.0
    assert float(define("ACN_MOTION_NONE")) == abi.ACN_MOTION_NONE == MM.NONE == 2.0
    body = re.search(r"typedef struct acn_motion_report\s*\{(.*?)\}\s*acn_motion_report;", text, re.S).group(1)
    assert re.findall(r"^\s*uint32_t\s+(\w+);", body, re.M) == [f[0] for f in abi.MotionReport._fields_] and C.sizeof(abi.MotionReport) == 16
    for word in ("1a OBJECT", "NO arithmetic", "SHAPE", "CHANGED", "OUTERMOST", "rax_prev^T * rax_cur", "shadow or reflection", "Clipping the history"):
        assert word in text, word
    assert "Motion per object is the caller's" not in text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "acn_reproject_moving" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the model: every row REST is reproject_model ----
@pytest.mark.parametrize("key", list(R.PARAM_SETS))
def test_all_rest_rows_are_the_model_of_acn_reproject(detmath_cpu, key):
    cur = R.tiled(131)
    cur[::3, 7] = 5                                                           # (more than one row is read)
    surf, st = R.prev_raster()
    surf[::2, 7] = np.where(surf[::2, 7] == 3, 5, surf[::2, 7])
    want, want_motion = R.reproject(detmath_cpu, cur, R.axis_params(), surf, st, **R.PARAM_SETS[key])
    detail = {}
    got, motion = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.rest_table(8), detail=detail, **R.PARAM_SETS[key])
    assert (bits(got) == bits(want)).all()
    both_nan = np.isnan(motion) & np.isnan(want_motion)
    assert ((bits(motion) == bits(want_motion)) | both_nan).all()
    assert (detail["state"][detail["hit"]] == 0).all() and 0 < T.empty(got).sum() < len(got)


# ---- answers known without the model ----
def centres(xs, ys, e):
    return np.stack([R.surface_record(x + 0.5, y + 0.5, e=e) for y in ys for x in xs])


def test_the_exact_shift_takes_the_record_of_the_next_pixel(detmath_cpu):
    surf, st = plain_raster()
    surf[:, 7] = MM.ROW_SHIFT
    cur = centres(range(R.PW - 1), range(R.PH), MM.ROW_SHIFT)
    detail = {}
    got, motion = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), detail=detail)
    want = np.stack([st[y * R.PW + x + 1] for y in range(R.PH) for x in range(R.PW - 1)])
    assert (bits(got) == bits(want)).all()
    assert np.array_equal(motion, [[x + 1.5, y + 0.5] for y in range(R.PH) for x in range(R.PW - 1)])
    assert (detail["state"] == 1).all() and (detail["valid"].sum(axis=1) == 1).all()
    off, _ = MM.reproject_moving(detmath_cpu, centres([R.PW - 1], range(R.PH), MM.ROW_SHIFT), R.axis_params(), surf, st, MM.hand_table())
    assert T.empty(off).all()                                                 # the last column came from beyond the raster


def test_the_exact_quarter_turn(detmath_cpu):
    """( a, 2, c ) -> ( -c, 2, a ): the centre of pixel ( x, y ) was on the centre of pixel ( y + 1, 4 - x ); N = ( 0, -1, 0 ) stays"""
    surf, st = plain_raster(seed=2)
    surf[:, 7] = MM.ROW_TURN
    xs, ys = range(5), range(R.PH)
    cur = centres(xs, ys, MM.ROW_TURN)
    detail = {}
    got, motion = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), normal_min=1.0, plane_tolerance=2.0 ** -40, detail=detail)
    want = np.stack([st[(4 - x) * R.PW + (y + 1)] for y in ys for x in xs])
    assert (bits(got) == bits(want)).all()
    assert np.array_equal(motion, [[y + 1.5, 4.5 - x] for y in ys for x in xs])
    assert detail["terms"]["normal"][detail["valid"]].all()                   # dot( Np, N' ) is exactly 1: the normal is as it was
    _, Pp, Np, _ = MM.rows_of(cur, MM.hand_table(), 32.0)
    assert np.array_equal(Pp, np.stack([-cur[:, 3], cur[:, 2], cur[:, 1]], axis=-1)) and np.array_equal(Np, cur[:, 4:7])


def test_a_rows_cap_beats_max_history_only_from_below(detmath_cpu):
    surf, st = plain_raster(n=128.0, seed=3)
    for row, n_want in ((MM.ROW_CAP4, 4.0), (MM.ROW_CAP64, 32.0), (MM.ROW_SHIFT, 32.0)):
        surf[:, 7] = row
        cur = centres([2], [2], row)
        got, _ = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), max_history=32.0)
        p = 2 * R.PW + 3
        assert got[0, 0] == n_want and np.array_equal(got[0, 1:4], st[p, 1:4]) and np.array_equal(got[0, 4:7], st[p, 4:7] * (n_want / 128.0))
    surf[:, 7] = MM.ROW_CAP64
    got, _ = MM.reproject_moving(detmath_cpu, centres([2], [2], MM.ROW_CAP64), R.axis_params(), surf, st, MM.hand_table(), max_history=100.0)
    assert got[0, 0] == 64.0
    t = MM.rest_table(8)
    for cap, n_want in ((np.inf, 32.0), (np.nan, 32.0), (0.5, 32.0), (-4.0, 32.0), (1.0, 1.0), (31.5, 31.5), (32.0, 32.0)):
        t[3, 13] = cap
        surf[:, 7] = 3
        got, _ = MM.reproject_moving(detmath_cpu, centres([2], [2], 3), R.axis_params(), surf, st, t)
        assert got[0, 0] == n_want, cap


def test_states_and_objects_of_the_hand_made_table(detmath_cpu):
    """NONE, a NaN state, an id beyond the table and an id of -1 are EMPTY with a NaN motion; an exit object selects the row where
    the enter object is -1; -0.0 is REST"""
    surf, st = MM.exit_raster()
    cur = MM.exit_and_outside_records()
    detail = {}
    got, motion = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), detail=detail)
    assert list(detail["state"]) == [0, 1, 1, 1, 2, 2, 1, 1, 2, 2, 2]
    none = detail["state"] == 2
    assert np.isnan(motion[none]).all() and T.empty(got[none]).all() and not np.isnan(motion[~none]).any()
    assert (bits(got[0]) == bits(st[2 * R.PW + 3])).all()                     # REST by the exit object: the record under the point
    assert (bits(got[1]) == bits(st[2 * R.PW + 4])).all()                     # the shift by the exit object: the record one pixel on
    t = MM.hand_table()
    t[MM.ROW_REST, 12] = -0.0
    again, _ = MM.reproject_moving(detmath_cpu, cur[:1], R.axis_params(), surf, st, t)
    assert (bits(again[0]) == bits(got[0])).all()


def test_a_rest_row_keeps_a_negative_zero_that_an_identity_would_lose(detmath_cpu):
    surf, st = plain_raster()
    r = R.surface_record(3.5, 2.5)
    r[3] = -0.0                                                               # P.z of the centre row
    _, P_rest, _, _ = MM.rows_of(r[None], MM.rest_table(8), 32.0)
    t = MM.rest_table(8)
    t[3] = MM.moved_row(np.eye(3), (0.0, 0.0, 0.0))
    _, P_id, _, _ = MM.rows_of(r[None], t, 32.0)
    assert np.signbit(P_rest[0, 2]) and not np.signbit(P_id[0, 2])


def test_the_tilt_meets_both_sides_of_the_normal_threshold(detmath_cpu):
    surf, st = MM.tilted_raster()
    surf[:, 7] = np.where(surf[:, 7] == 3, MM.ROW_TILT, surf[:, 7])
    cur = MM.tilt_records()
    for nmin, at_x in ((None, 2), (0.875, 5)):
        detail = {}
        got, _ = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), normal_min=nmin, detail=detail)
        heavy = np.argmax(detail["weights"], axis=1)                          # Pp meets a pixel centre to rounding: one tap has all but 1e-15 of the weight
        normal = detail["terms"]["normal"][np.arange(len(cur)), heavy]
        on, beyond = 2 * at_x, 2 * (at_x + 1)                                 # (the records come in pairs, y = 1 and 2 per x)
        assert detail["weights"].max(axis=1).min() > 1.0 - 1e-12
        assert normal[on] and detail["valid"][on, heavy[on]] and not normal[beyond], nmin
        assert normal[0] and normal[2] and not T.empty(got[0:1]).all()        # the tilted normal itself


@pytest.mark.parametrize("key", list(R.PARAM_SETS))
def test_the_hand_made_cases_show_every_state_and_both_outcomes_of_every_term(detmath_cpu, key):
    """what the GPU test compares bit for bit: the cases of motion_model.hand_cases under the three parameter sets"""
    details = []
    for name, cur, surf, st in MM.hand_cases():
        detail = {}
        got, motion = MM.reproject_moving(detmath_cpu, cur, R.axis_params(), surf, st, MM.hand_table(), detail=detail, **R.PARAM_SETS[key])
        details.append(detail)
        assert len(cur) >= MM.N_HAND and 0 < T.empty(got).sum() <= len(got), name
        assert (got[~T.empty(got), 0] >= 1.0).all() and (got[T.empty(got)] == 0).all()
        assert np.array_equal(np.isnan(motion[:, 0]), ~detail["projected"])
    decided = MM.TERMS if key != "all kinds, no normal test" else tuple(t for t in MM.TERMS if t not in ("normal", "plane"))
    assert MM.coverage(details, decided) == []
    caps = np.concatenate([d["cap"] for d in details])
    call_cap = R.PARAM_SETS[key].get("max_history", R.DEFAULT_MAX_HISTORY)
    assert (caps == call_cap).any() and ((caps == 4.0).any() or call_cap <= 4.0) and not (caps == 64.0).any()


# ---- acn_motion_from_scenes through ctypes against the model ----
def compare_tables(prev, cur, cap=None):
    got, rep = A.motion_from_scenes(prev, cur, cap)
    want, want_rep = MM.motion_from_scenes(prev, cur, 0.0 if cap is None else cap)
    assert (bits(got) == bits(want)).all(), (got, want)
    assert rep == want_rep
    assert rep["rest"] + rep["moved"] + rep["none"] == cur.c.n_nodes
    return got, rep


def test_identical_scenes_are_all_rest():
    _, a = MM.build_pose()
    _, b = MM.build_pose()
    table, rep = compare_tables(a, b)
    assert rep == dict(rest=a.c.n_nodes, moved=0, none=0, same_shape=True) and (table == 0).all()


def test_the_ball_turned_and_shifted_is_moved():
    turn, shift = 10.0, (0.15, 0.0, 0.0)
    _, a = MM.build_pose()
    _, b = MM.build_pose(turn_deg=turn, shift=shift)
    table, rep = compare_tables(a, b, cap=8.0)
    ball = MM.ball_node(a)
    assert rep == dict(rest=a.c.n_nodes - 1, moved=1, none=0, same_shape=True)
    m = table[ball]
    assert m[12] == MM.MOVED and m[13] == 8.0 and (m[14:] == 0).all()
    Am, t = m[0:9].reshape(3, 3), m[9:12]
    c, s = np.cos(np.radians(turn)), np.sin(np.radians(turn))
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = np.array(MM.BALL_CENTRE)
    for u in ((1.0, 0.0, 0.0), (0.0, -0.6, 0.8), (-0.48, 0.64, -0.6)):
        p_prev = centre + 0.9 * np.array(u)
        p_cur = Rz @ (p_prev - centre) + centre + np.array(shift)             # by hand: turned about the centre, then shifted
        err = float(np.abs(Am @ p_cur + t - p_prev).max())
        assert err <= 1e-12, err
    for i in range(a.c.n_nodes):
        if i != ball:
            assert (table[i] == 0).all()


@pytest.mark.parametrize("change", [dict(radius=0.8), dict(ball_colour=(0.9, 0.25, 0.2)), dict(skew=True)])
def test_a_changed_or_skewed_object_has_no_history(change):
    _, a = MM.build_pose()
    _, b = MM.build_pose(turn_deg=5.0 if "skew" in change else 0.0, **change)
    table, rep = compare_tables(a, b)
    ball = MM.ball_node(a)
    assert table[ball, 12] == MM.NONE and (np.delete(table[ball], 12) == 0).all()
    assert rep == dict(rest=a.c.n_nodes - 1, moved=0, none=1, same_shape=True)
    if "skew" in change:                                                      # the same turn without the skew is MOVED
        _, c = MM.build_pose(turn_deg=5.0)
        assert compare_tables(a, c)[0][ball, 12] == MM.MOVED
        assert compare_tables(b, c)[0][ball, 12] == MM.NONE                   # ... and a skewed previous frame is refused alike


def test_a_changed_texture_has_no_history():
    _, a = MM.build_pose()
    _, b = MM.build_pose()
    tex = b.node(MM.ball_node(b)).texture
    b.c.textures[tex].scale = 5.0
    table, rep = compare_tables(a, b)
    assert table[MM.ball_node(a), 12] == MM.NONE and rep["none"] == 1


def test_another_node_count_is_another_shape():
    _, a = MM.build_pose()
    _, b = MM.build_pose(extra=True)
    table, rep = compare_tables(a, b)
    assert rep == dict(rest=0, moved=0, none=b.c.n_nodes, same_shape=False) and len(table) == b.c.n_nodes and (table[:, 12] == MM.NONE).all()


def test_nodes_below_a_scale_node_take_its_row():
    _, a = MM.build_pose(scaled=(0.3, 0.0))
    _, b = MM.build_pose(scaled=(0.3, 20.0))
    scale = MM.matter_elems(a)[-1]
    inner = a.node(scale).child0
    assert a.node(scale).type == abi.ACN_SCALE and a.node(inner).type == abi.ACN_SPHERE
    table, rep = compare_tables(a, b, cap=2.0)
    assert table[scale, 12] == MM.MOVED and (bits(table[inner]) == bits(table[scale])).all()
    assert rep == dict(rest=a.c.n_nodes - 2, moved=2, none=0, same_shape=True)
    table, rep = compare_tables(a, a)
    assert rep["rest"] == a.c.n_nodes
    _, c = MM.build_pose(scaled=(0.35, 20.0))                                 # the inner sphere changed: the whole scaled object is stale
    table, rep = compare_tables(a, c)
    assert table[scale, 12] == MM.NONE and table[inner, 12] == MM.NONE and rep == dict(rest=a.c.n_nodes - 2, moved=0, none=2, same_shape=True)
    _, d = MM.build_pose(scaled=(0.35, 0.0))                                  # ... and so it is where the scale node stayed
    table, rep = compare_tables(a, d)
    assert table[scale, 12] == MM.NONE and table[inner, 12] == MM.NONE


def test_motion_from_scenes_refusals():
    _, a = MM.build_pose()
    n = a.c.n_nodes
    table = np.full((n, 16), 7.25)
    rep = abi.MotionReport(9, 9, 9, 9)
    ref = C.byref

    def refused(call, word):
        assert call() == abi.ACN_ERR_ARG
        msg = hip.acn_last_error().decode()
        assert word in msg, msg
        assert (table == 7.25).all() and (rep.n_rest, rep.n_moved, rep.n_none, rep.same_shape) == (9, 9, 9, 9)

    refused(lambda: hip.acn_motion_from_scenes(None, ref(a.c), 0.0, table.ctypes.data, ref(rep)), "prev")
    refused(lambda: hip.acn_motion_from_scenes(ref(a.c), None, 0.0, table.ctypes.data, ref(rep)), "cur")
    refused(lambda: hip.acn_motion_from_scenes(ref(a.c), ref(a.c), 0.0, None, ref(rep)), "out_table")
    for bad in (float("nan"), -1.0, -0.5, 0.5, 1e-300, float("-inf")):
        refused(lambda: hip.acn_motion_from_scenes(ref(a.c), ref(a.c), bad, table.ctypes.data, ref(rep)), "moved_max_history")
    for good in (0.0, 1.0, 8.0, float("inf")):
        assert hip.acn_motion_from_scenes(ref(a.c), ref(a.c), good, table.ctypes.data, None) == abi.ACN_OK   # the report is optional
    assert (table == 0).all()
    for f in (hip.acn_reproject_moving, hip.acn_reproject_moving_dev):       # the entry points refuse a null handle before anything else
        buf = np.full((4, 16), 7.25)
        prm = R.axis_params()
        assert f(None, buf.ctypes.data, 4, ref(prm), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4, None, buf.ctypes.data, None, None) == abi.ACN_ERR_ARG
        assert "handle" in hip.acn_last_error().decode() and (buf == 7.25).all()


# ---- rigid_copy against the host library ----
def small_scene(which, move):
    """a floor and one object; move: the object turned 33 degrees about z and 10 about x through `pivot`, then shifted, by the host library"""
    sc = A.Scene()
    sc.set(image_width=16, image_height=12)
    floor = host.acn_obj_plane_s_create()
    host.acn_obj_move(floor, A.v3(0, 0, -1))
    if which == "ball":
        o = host.acn_obj_sphere_s_create(0.9)
        m = host.acn_rotx(25)
        host.acn_obj_rotate(o, C.byref(m))
        host.acn_obj_move(o, A.v3(-1.2, 0.3, 0.1))
        host.acn_obj_set_envelope(o, A.v3(-1.2, 0.3, 0.1), 1.0)
    elif which == "torus":
        o = host.acn_obj_torus_create(0.5, 0.18)
        host.acn_obj_move(o, A.v3(1.7, -0.6, -0.5))
    else:
        a, b, c = host.acn_obj_sphere_s_create(0.7), host.acn_obj_squaroid_s_create_ellipsoid(0.5, 0.5, 0.8), host.acn_obj_sphere_s_create(0.6)
        host.acn_obj_move(b, A.v3(0.3, 0.1, 0.0))
        host.acn_obj_move(c, A.v3(-0.2, 0.2, 0.1))
        lst = (C.c_void_p * 3)(a, b, c)
        o = host.acn_create_inside_composite(lst, 3)
        for part in (a, b, c):
            host.acn_obj_discard(part)
        host.acn_obj_move(o, A.v3(0.4, 1.0, 0.2))
    if move:
        rotation, pivot, shift = move
        if rotation is not None:
            if pivot is not None:
                host.acn_obj_move(o, A.v3(*[-v for v in pivot]))
            host.acn_obj_rotate(o, C.byref(rotation))
            if pivot is not None:
                host.acn_obj_move(o, A.v3(*pivot))
        if shift is not None:
            host.acn_obj_move(o, A.v3(*shift))
    for obj in (floor, o):
        sc.push(obj)
        host.acn_obj_discard(obj)
    return sc.flatten()


@pytest.mark.parametrize("which", ["ball", "torus", "pair"])
def test_rigid_copy_is_the_host_librarys_move_and_rotate(which):
    rz, rx = host.acn_rotz(33.0), host.acn_rotx(10.0)
    rows = MM.matrix_rows(rz)
    base = small_scene(which, None)
    node = MM.matter_elems(base)[1]
    if which == "pair":
        assert base.node(node).type == abi.ACN_PAIR_INSIDE and base.c.n_nodes >= 7
    before = base.nodes_bytes()
    for pivot, shift, rotation in (((0.4, 1.0, 0.2), (0.15, -0.05, 0.3), rz), (None, (1.0, 2.0, 3.0), rz), ((1.0, 0.0, -1.0), None, rx), (None, (0.5, 0.0, 0.0), None)):
        want = small_scene(which, (rotation, pivot, shift))
        got = A.rigid_copy(base, node, None if rotation is None else MM.matrix_rows(rotation), pivot, shift)
        assert got.nodes_bytes() == want.nodes_bytes(), (which, pivot, shift)
        assert got.nodes_bytes() != before and base.nodes_bytes() == before   # a copy: the original stays
        assert list(got.c.elems[:got.c.n_elems]) == list(base.c.elems[:base.c.n_elems]) and got.c.matter_root == base.c.matter_root
    assert A.rigid_copy(base, node).nodes_bytes() == before
    assert rows == MM.matrix_rows(rz)
    with pytest.raises(ValueError):
        A.rigid_copy(base, base.c.n_nodes)
    # and the table of the copy names the object and nothing else
    moved = A.rigid_copy(base, node, rows, (0.4, 1.0, 0.2), (0.1, 0.0, 0.0))
    table, rep = compare_tables(base, moved)
    reached = {i for i, prp in subtree(base, node) if prp}
    assert {int(i) for i in np.flatnonzero(table[:, 12] == MM.MOVED)} == reached and rep["none"] == 0


# ---- the two rendered frames of the GPU test, on the oracle's first hits ----
def test_the_rendered_pose_gives_the_ball_a_history_only_through_its_motion(oracle, detmath_cpu):
    """The pose of tests/test_gpu_reproject_moving.py: the ball turned 10 degrees about z through its centre and shifted by ( 0.15, 0, 0 ),
    the camera orbited by 2 degrees, 96 x 72.  Of the ELIGIBLE positions on the ball more than half take a history through the table,
    and strictly more than with the world taken to be at rest: a condition on the input, confirmed here before the device is asked"""
    fr = MM.two_frames()
    rays = lambda params: F.camera_rays(params, A.main_pass_positions(96, 72))
    prev_surf, _ = F.first_hit(oracle, fr["prev_flat"], rays(fr["prev_params"]))
    cur, _ = F.first_hit(oracle, fr["cur_flat"], rays(fr["cur_params"]))
    prev_st = MM.synthetic_stats(len(prev_surf))
    table, rep = A.motion_from_scenes(fr["prev_flat"], fr["cur_flat"])
    assert rep["moved"] == 1 and rep["none"] == 0
    ball = MM.ball_node(fr["cur_flat"])
    detail = {}
    moving, _ = MM.reproject_moving(detmath_cpu, cur, fr["prev_params"], prev_surf, prev_st, table, detail=detail)
    at_rest, _ = R.reproject(detmath_cpu, cur, fr["prev_params"], prev_surf, prev_st)
    on_ball = detail["eligible"] & (cur[:, 7] == ball)
    share, share_rest = float((~T.empty(moving))[on_ball].mean()), float((~T.empty(at_rest))[on_ball].mean())
    print(f"{int(on_ball.sum())} ELIGIBLE positions on the ball: {share:.3f} take a history through the table, {share_rest:.3f} with the world at rest")
    assert on_ball.sum() >= 100 and share > 0.5 and share > share_rest
    off_ball = detail["eligible"] & (cur[:, 7] != ball)
    assert (bits(moving[off_ball]) == bits(at_rest[off_ball])).all()          # everything else is at rest: the same records


# ---- the host-side unit under the sanitizers ----
def test_host_unit_in_a_sanitized_program(tmp_path):
    """csrc/acn_motion_host.h compiled with tests/csrc/motion_cpu.cpp into a program of its own with -fsanitize=address,undefined;
    nothing sanitized is loaded here"""
    exe = tmp_path / "motion_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "motion_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

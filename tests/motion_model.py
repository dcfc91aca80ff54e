"""numpy model of acn_reproject_moving and of acn_motion_from_scenes (include/actinon_hip.h): the expressions of the header in the header's
order, beside reproject_model, whose projection, records and patterns it uses.  The device and the host library are compared with
it bit for bit.  Also the hand-made motion table of the tests, the previous rasters that go with its rows, and the pose scene: the
recipe of scenes_util.build_textured with a pose for the ball."""
import ctypes as C

import numpy as np

import actinon_amd as A
import lens_model as M
import reproject_model as R
import stats_model as T
from actinon_amd import abi

STRIDE = 16
REST, MOVED, NONE = 0.0, 1.0, 2.0
SURF, STATS = R.SURF, R.STATS
TERMS = ("inside", "weight", "not_empty", "tap_hit", "match", "normal", "plane")


def rest_table(n):
    """n rows REST with m[ 13 ] = 0"""
    return np.zeros((n, STRIDE))


def moved_row(Amat, t, cap=0.0):
    m = np.zeros(STRIDE)
    m[0:9] = np.asarray(Amat, dtype=np.float64).reshape(9)
    m[9:12] = t
    m[12], m[13] = MOVED, cap
    return m


def rows_of(cur, table, cap):
    """1a OBJECT -> ( state [n] as 0 REST / 1 MOVED / 2 NONE, Pp [n,3], Np [n,3], cap [n] )"""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, STRIDE)
    e, x = R.int32(cur[:, 7]), R.int32(cur[:, 8])
    oid = np.where(e >= 0, e, x).astype(np.int64)
    inside = (oid >= 0) & (oid < len(table))
    row = table[np.where(inside, oid, 0)]
    with np.errstate(all="ignore"):
        moved = inside & (row[:, 12] == MOVED)
        rest = inside & (row[:, 12] == REST)
        state = np.where(moved, 1, np.where(rest, 0, 2))
        P, N = cur[:, 1:4], cur[:, 4:7]
        Ax, Ay, Az, t = row[:, 0:3], row[:, 3:6], row[:, 6:9], row[:, 9:12]
        Pm = np.stack([M.dot(Ax, P) + t[:, 0], M.dot(Ay, P) + t[:, 1], M.dot(Az, P) + t[:, 2]], axis=-1)
        Nm = np.stack([M.dot(Ax, N), M.dot(Ay, N), M.dot(Az, N)], axis=-1)
        own = inside & (row[:, 13] >= 1.0) & (row[:, 13] < cap)
    return state, np.where(moved[:, None], Pm, P), np.where(moved[:, None], Nm, N), np.where(own, row[:, 13], cap)


def reproject_moving(lib, cur, prev_params, prev_surf, prev_stats, motion, reject_kinds=None, max_hops=None, normal_min=None,
                     plane_tolerance=None, max_history=None, detail=None):
    """-> ( stats [n,8], motion [n,2] ).  The steps of reproject_model.reproject with 1a, Pp, Np and the row's cap.  detail receives
    `hit`, `state`, `projected`, `eligible`, `cap` [n], `valid` and `weights` [n,4] and `terms`: per VALID term its outcome [n,4]"""
    reject = R.DEFAULT_REJECT_KINDS if reject_kinds is None else int(reject_kinds)
    hops_max = R.DEFAULT_MAX_HOPS if max_hops is None else int(max_hops)
    nmin = R.DEFAULT_NORMAL_MIN if normal_min in (None, 0) else float(normal_min)
    tol = R.DEFAULT_PLANE_TOLERANCE if plane_tolerance in (None, 0) else float(plane_tolerance)
    call_cap = R.DEFAULT_MAX_HISTORY if max_history in (None, 0) else float(max_history)
    cur = np.ascontiguousarray(cur, dtype=np.float64).reshape(-1, SURF)
    W, H = int(prev_params.image_width), int(prev_params.image_height)
    ps = np.ascontiguousarray(prev_surf, dtype=np.float64).reshape(H * W, SURF)
    pt = np.ascontiguousarray(prev_stats, dtype=np.float64).reshape(H * W, STATS)
    n = len(cur)
    cam = M.Camera(lib, prev_params)
    with np.errstate(all="ignore"):
        hit = cur[:, 0] < np.inf                                              # 1
        state, Pp, Np, cap = rows_of(cur, motion, call_cap)                   # 1a
        known = hit & (state != 2)
        q, _, ok = R.project(cam, Pp)                                         # 2
        projected = known & ok
        motion_out = np.where(projected[:, None], q, np.nan)
        eligible = projected & ((R.int32(cur[:, 12]).astype(np.uint32) & np.uint32(reject)) == 0) & (R.int32(cur[:, 13]) <= hops_max)   # 3
        qx, qy = np.where(projected, q[:, 0], 0.0), np.where(projected, q[:, 1], 0.0)
        fx, fy = qx - 0.5, qy - 0.5                                           # 4
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        key = R.int32(cur[:, [7, 8, 13]])
        pkey = R.int32(ps[:, [7, 8, 13]])
        pempty = T.empty(pt)
        limit = tol * cur[:, 0]
        sw, sn, sm, s2 = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        valid = np.zeros((n, 4), dtype=bool)
        weights = np.zeros((n, 4))
        terms = {name: np.zeros((n, 4), dtype=bool) for name in TERMS}
        for k in range(4):
            x, y = (x0 + 1.0 if k & 1 else x0), (y0 + 1.0 if k & 2 else y0)
            w = (tx if k & 1 else 1.0 - tx) * (ty if k & 2 else 1.0 - ty)
            inside = (x >= 0.0) & (x < float(W)) & (y >= 0.0) & (y < float(H))
            p = np.where(inside, y, 0.0).astype(np.int64) * W + np.where(inside, x, 0.0).astype(np.int64)   # 5
            r, t = ps[p], pt[p]
            D = r[:, 1:4] - Pp
            term = dict(inside=inside, weight=w > 0.0, not_empty=~pempty[p], tap_hit=r[:, 0] < np.inf, match=(pkey[p] == key).all(axis=1),
                        normal=M.dot(Np, r[:, 4:7]) >= nmin, plane=np.abs(M.dot(Np, D)) <= limit)
            v = eligible.copy()
            for name in TERMS:
                terms[name][:, k] = term[name]
                v &= term[name]
            valid[:, k] = v
            weights[:, k] = w
            sw = np.where(v, sw + w, sw)                                      # 6
            sn = np.where(v, sn + w * t[:, 0], sn)
            sm = np.where(v[:, None], sm + w[:, None] * t[:, 1:4], sm)
            s2 = np.where(v[:, None], s2 + w[:, None] * t[:, 4:7], s2)
        any_valid = valid.any(axis=1)
        cnt, mean, m2 = sn / sw, sm / sw[:, None], s2 / sw[:, None]
        over = cnt > cap
        m2 = np.where(over[:, None], m2 * (cap / cnt)[:, None], m2)
        cnt = np.where(over, cap, cnt)
    out = np.zeros((n, STATS))
    out[any_valid, 0] = cnt[any_valid]
    out[any_valid, 1:4] = mean[any_valid]
    out[any_valid, 4:7] = m2[any_valid]
    if detail is not None:
        detail.update(hit=hit, state=state, projected=projected, eligible=eligible, valid=valid, terms=terms, weights=weights, cap=cap)
    return out, motion_out


# ---- the hand-made table: eight rows, and what goes with them ----
SHIFT_A, SHIFT_T = np.eye(3), (1.0, 0.0, 0.0)                                 # pixel ( x, y ) -> pixel ( x + 1, y )
TURN_A, TURN_T = [[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], (0.0, 0.0, 0.0)   # ( a, 2, c ) -> ( -c, 2, a ): a quarter turn about the view axis
TILT = 0.004                                                                  # radians about x: off the plane by 0.008 per unit of height
ROW_REST, ROW_SHIFT, ROW_TURN, ROW_TILT, ROW_NONE, ROW_NAN, ROW_CAP4, ROW_CAP64 = range(8)


def tilt_matrix():
    c, s = np.cos(TILT), np.sin(TILT)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def hand_table():
    """REST; the exact shift; the exact quarter turn; a tilt about x through the raster's centre point; NONE; a NaN state; the shift
    with a cap of 4; the shift with a cap of 64"""
    t = np.zeros((8, STRIDE))
    t[ROW_SHIFT] = moved_row(SHIFT_A, SHIFT_T)
    t[ROW_TURN] = moved_row(TURN_A, TURN_T)
    Am = tilt_matrix()
    centre = np.array([0.0, R.DEPTH, 0.0])
    t[ROW_TILT] = moved_row(Am, centre - Am @ centre)
    t[ROW_NONE, 12] = NONE
    t[ROW_NAN, 12] = np.nan
    t[ROW_CAP4] = moved_row(SHIFT_A, SHIFT_T, cap=4.0)
    t[ROW_CAP64] = moved_row(SHIFT_A, SHIFT_T, cap=64.0)
    return t


def relabel(records, obj, other):
    """the records with enter object 3 -> obj and 4 -> other (the two enter objects of reproject_model's records)"""
    out = np.array(records, dtype=np.float64, copy=True)
    e = out[:, 7].copy()
    out[e == 3, 7] = obj
    out[e == 4, 7] = other
    return out


def factor_for(a, target):
    """u with fl( a * u ) == target: |a| < 1 steps the product by less than its spacing, so every target near a * u is met"""
    u = target / a
    for _ in range(64):
        got = a * u
        if got == target:
            return u
        u = np.nextafter(u, -np.inf if (got > target) == (a > 0) else np.inf)
    raise AssertionError("no factor")


def tilted_raster(nmins=(R.DEFAULT_NORMAL_MIN, 0.875)):
    """reproject_model.prev_raster with the previous normals of row y = 1 tilted to match ROW_TILT: with Np = A * ( 0, -1, 0 ), pixels
    ( 0, 1 ) and ( 1, 1 ) hold Np itself, and for each normal_min of `nmins` one pixel a normal with dot( Np, N' ) == normal_min exactly
    and the next one ulp below it: ( 2, 1 ), ( 3, 1 ) and ( 5, 1 ), ( 6, 1 )"""
    surf, st = R.prev_raster()
    Am = tilt_matrix()
    N = np.array([0.0, -1.0, 0.0])
    Np = np.array([M.dot(Am[0], N), M.dot(Am[1], N), M.dot(Am[2], N)])
    at = lambda x, y: y * R.PW + x
    for x in (0, 1):
        surf[at(x, 1), 4:7] = Np
        st[at(x, 1), 0] = 3.0
    for x, nmin in zip((2, 5), nmins):
        for dx, target in ((0, nmin), (1, np.nextafter(nmin, 0.0))):
            u = factor_for(Np[1], target)
            Nq = np.array([0.0, u, 0.0])
            assert M.dot(Np, Nq) == target
            surf[at(x + dx, 1), 4:7] = Nq
            st[at(x + dx, 1), 0] = 3.0
    return surf, st


def tilt_records():
    """current records of ROW_TILT's object aimed at the pixels of tilted_raster's row y = 1 and around: the pixel whose centre Pp meets
    is found by inverting the row"""
    t = hand_table()[ROW_TILT]
    Am, tt = t[0:9].reshape(3, 3), t[9:12]
    out = []
    for x in range(R.PW):
        for y in (1, 2):
            target = R.point_at(x + 0.5, y + 0.5)
            r = R.surface_record(x + 0.5, y + 0.5, e=ROW_TILT)
            r[1:4] = Am.T @ (target - tt)                                     # to rounding: the taps' weights are then close to 1 and 0
            out.append(r)
    return np.stack(out)


def exit_and_outside_records():
    """records whose enter object is -1 and whose exit object selects the row; an id beyond the table; an id of -1"""
    out = []
    for row in range(8):
        out.append(R.surface_record(3.5, 2.5, e=-1, x=row))
    out.append(R.surface_record(3.5, 2.5, e=8))
    out.append(R.surface_record(3.5, 2.5, e=-1, x=8))
    out.append(R.surface_record(3.5, 2.5, e=-1, x=-1))
    return np.stack(out)


def exit_raster():
    """reproject_model.prev_raster whose pixels ( 3, 2 ) and ( 4, 2 ) show enter -1 with the exit objects ROW_REST and ROW_SHIFT"""
    surf, st = R.prev_raster()
    at = lambda x, y: y * R.PW + x
    surf[at(3, 2), 7:9] = (-1, ROW_REST)
    surf[at(4, 2), 7:9] = (-1, ROW_SHIFT)
    return surf, st


N_HAND = 64 * 2 + 3                                                           # a wavefront boundary and a tail


def hand_cases():
    """-> [( name, cur [n,16], prev surface [35,16], prev statistics [35,8] )] for hand_table().  A tap must show the object of the
    current record (the MATCH rule), so the patterns of reproject_model meet every row in a raster of that row's object: case k has
    enter object 3 -> k and 4 -> k + 1 in the N_HAND tiled patterns and in the raster; the tilt's case has the tilted raster and the
    records aimed at it on top.  The last case mixes the rows over the lanes -- position i shows object i % 8 -- and holds the
    records of exit objects and of ids outside the table"""
    out = []
    for k in range(8):
        surf, st = tilted_raster() if k == ROW_TILT else R.prev_raster()
        cur = relabel(R.tiled(N_HAND), k, (k + 1) % 8)
        if k == ROW_TILT:
            cur = np.concatenate([cur, tilt_records()])
        out.append((f"object {k}", cur, relabel(surf, k, (k + 1) % 8), st))
    extra = exit_and_outside_records()
    mixed = R.tiled(N_HAND - len(extra))
    hit = mixed[:, 0] < np.inf
    mixed[hit, 7] = (np.arange(len(mixed)) % 8)[hit]
    surf, st = exit_raster()
    out.append(("mixed rows, exit objects, ids outside", np.concatenate([mixed, extra]), surf, st))
    return out


def coverage(details, terms=TERMS):
    """what a list of `detail` dicts shows: every state, and both outcomes of every VALID term on the taps of ELIGIBLE positions that
    lie in the image (whose records are read), with a valid and an invalid tap among them -> list of what is missing"""
    missing = []
    states = np.concatenate([d["state"][d["hit"]] for d in details])
    for s, name in enumerate(("REST", "MOVED", "NONE")):
        if not (states == s).any():
            missing.append(name)
    for name in terms:
        seen = set()
        for d in details:
            read = d["eligible"][:, None] & (d["terms"]["inside"] | (name == "inside"))
            seen |= set(np.unique(d["terms"][name][read]).tolist())
        if seen != {True, False}:
            missing.append((name, sorted(seen)))
    if not any(d["valid"].any() for d in details) or all(d["valid"][d["eligible"]].all() for d in details):
        missing.append("valid")
    return missing


# ---- acn_motion_from_scenes ----
def node_array(flat):
    return np.frombuffer(flat.nodes_bytes(), dtype=np.uint8).reshape(flat.c.n_nodes, C.sizeof(abi.Node))


def texture_bytes(flat, index):
    if not 0 <= index < flat.c.n_textures:
        return None
    return C.string_at(C.addressof(flat.c.textures[index]), C.sizeof(abi.Texture))


def texture_same(prev, cur, i):
    a, b = prev.node(i).texture, cur.node(i).texture
    if a != b:
        return False
    if b < 0:
        return True
    ta, tb = texture_bytes(prev, a), texture_bytes(cur, b)
    return ta is not None and ta == tb


def orthonormal(rax):
    r = np.asarray(rax, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        worst = max(abs(float(M.dot(r[i], r[j])) - (1.0 if i == j else 0.0)) for i in range(3) for j in range(3))
    return worst <= 1e-9


def children(flat, i):
    nd = flat.node(i)
    if nd.type == abi.ACN_COMPOUND:
        return flat.elems_of(i)
    if nd.type in (abi.ACN_PAIR_INSIDE, abi.ACN_PAIR_OUTSIDE):
        return [nd.child0, nd.child1]
    if nd.type in (abi.ACN_NEG, abi.ACN_SCALE):
        return [nd.child0]
    return []


def motion_from_scenes(prev, cur, moved_max_history=0.0):
    """-> ( table [n,16], report ) by the rules of the header in the header's order"""
    n = cur.c.n_nodes
    none_row = np.zeros(STRIDE); none_row[12] = NONE
    table = np.tile(none_row, (n, 1))
    f = lambda flat, i, name: getattr(flat.node(i), name)
    same = (prev.c.n_nodes == n and prev.c.n_elems == cur.c.n_elems and prev.c.light_root == cur.c.light_root and prev.c.matter_root == cur.c.matter_root
            and list(prev.c.elems[:prev.c.n_elems]) == list(cur.c.elems[:cur.c.n_elems])
            and all(f(prev, i, k) == f(cur, i, k) for i in range(n) for k in ("type", "child0", "child1")))
    if same:
        off = {name: getattr(abi.Node, name).offset for name in ("prm", "color", "pad_", "pos", "rax", "env_pos")}
        pb, cb = node_array(prev), node_array(cur)
        span = lambda b, i, a, z: bytes(b[i, a:z])
        for i in range(n):
            changed = (span(pb, i, off["prm"], off["color"]) != span(cb, i, off["prm"], off["color"])
                       or span(pb, i, off["color"], off["pad_"]) != span(cb, i, off["color"], off["pad_"])
                       or f(prev, i, "sdf_kind") != f(cur, i, "sdf_kind") or f(prev, i, "cycles") != f(cur, i, "cycles") or not texture_same(prev, cur, i))
            if changed:
                continue
            if span(pb, i, off["pos"], off["env_pos"]) == span(cb, i, off["pos"], off["env_pos"]):      # pos and rax lie side by side
                table[i] = 0.0
                continue
            rp, rc = np.array(f(prev, i, "rax")[:]).reshape(3, 3), np.array(f(cur, i, "rax")[:]).reshape(3, 3)
            pp, pc = np.array(f(prev, i, "pos")[:]), np.array(f(cur, i, "pos")[:])
            if not (orthonormal(rp) and orthonormal(rc)):
                continue
            Am = np.array([[(rp[0, a] * rc[0, b] + rp[1, a] * rc[1, b]) + rp[2, a] * rc[2, b] for b in range(3)] for a in range(3)])
            t = np.array([pp[a] - ((Am[a, 0] * pc[0] + Am[a, 1] * pc[1]) + Am[a, 2] * pc[2]) for a in range(3)])
            table[i] = moved_row(Am, t, moved_max_history)
        outer = {}
        todo = [(r, -1) for r in dict.fromkeys((cur.c.light_root, cur.c.matter_root))]
        seen = {r for r, _ in todo}
        while todo:
            i, above = todo.pop()
            below = above if above >= 0 else (i if cur.node(i).type == abi.ACN_SCALE else -1)
            for k in children(cur, i):
                if k not in seen:
                    seen.add(k)
                    outer[k] = below
                    todo.append((k, below))
        unequal = {s for k, s in outer.items() if s >= 0 and (bytes(pb[k]) != bytes(cb[k]) or not texture_same(prev, cur, k))}
        for k, s in outer.items():
            if s >= 0:
                table[k] = none_row if s in unequal else table[s]
        for s in unequal:
            table[s] = none_row
    state = table[:, 12]
    report = dict(rest=int((state == REST).sum()), moved=int((state == MOVED).sum()), none=int(((state != REST) & (state != MOVED)).sum()), same_shape=bool(same))
    return table, report


# ---- the pose scene ----
BALL_ELEM, TORUS_ELEM = 1, 3                                                  # root elements of matter (the light goes to the light root): floor, ball, egg, torus
BALL_CENTRE = (-1.2, 0.0, 0.0)


def rotz(deg):
    return A.host.acn_rotz(float(deg))


def matrix_rows(m):
    return [[m.x.x, m.x.y, m.x.z], [m.y.x, m.y.y, m.y.z], [m.z.x, m.z.y, m.z.z]]


def build_pose(turn_deg=0.0, shift=(0.0, 0.0, 0.0), radius=0.9, ball_colour=(0.9, 0.2, 0.2), skew=False, extra=False, scaled=None, width=96, height=72):
    """scenes_util.build_textured's recipe with a pose for the ball: turned by turn_deg about z through its centre, then shifted.
    radius, ball_colour: a changed object; extra: one more sphere (another node count); scaled: None, or ( inner radius, z turn of the
    scale node in degrees ): a sphere under an ACN_SCALE node pushed last -> ( Scene, Flat )"""
    host = A.host
    sc = A.Scene()
    sc.set(image_width=width, image_height=height, gamma=1.0, trace_depth=25, trace_min_intensity=0.03, direct_samples=20,
           path_samples=16, max_path_length=4.0, camera_position=(0, -8, 2), camera_view_direction=(0, 8, -2),
           camera_top_direction=(0, 0, 1), camera_focal_length=3, background_color=(0.3, 0.35, 0.4))
    objs = []
    light = host.acn_obj_sphere_s_create(0.6)
    host.acn_obj_set_radiance(light, 25.0)
    host.acn_obj_set_texture_field_chess(light, A.v3(1.0, 0.9, 0.8), A.v3(0.8, 0.9, 1.0), 3.0)
    host.acn_obj_move(light, A.v3(-2, -3, 5))
    objs.append(light)
    floor = host.acn_obj_plane_s_create()
    host.acn_obj_set_material(floor, b"diffuse_polished")
    host.acn_obj_set_texture_field_chess(floor, A.v3(0.9, 0.9, 0.9), A.v3(0.2, 0.2, 0.25), 1.0)
    host.acn_obj_move(floor, A.v3(0, 0, -1))
    objs.append(floor)
    ball = host.acn_obj_sphere_s_create(radius)
    host.acn_obj_set_material(ball, b"diffuse")
    host.acn_obj_set_texture_field_chess(ball, A.v3(*ball_colour), A.v3(0.95, 0.9, 0.3), 4.0)
    m = host.acn_rotx(25)
    host.acn_obj_rotate(ball, C.byref(m))
    host.acn_obj_move(ball, A.v3(*BALL_CENTRE))
    if turn_deg:
        host.acn_obj_move(ball, A.v3(*[-v for v in BALL_CENTRE]))
        m = rotz(turn_deg)
        host.acn_obj_rotate(ball, C.byref(m))
        host.acn_obj_move(ball, A.v3(*BALL_CENTRE))
    if any(shift):
        host.acn_obj_move(ball, A.v3(*shift))
    objs.append(ball)
    egg = host.acn_obj_squaroid_s_create_ellipsoid(0.5, 0.5, 0.8)
    host.acn_obj_set_material(egg, b"mirror")
    host.acn_obj_set_texture_field_plain(egg, A.v3(0.3, 0.8, 0.4))
    host.acn_obj_move(egg, A.v3(0.6, 0.5, -0.2))
    objs.append(egg)
    tor = host.acn_obj_torus_create(0.5, 0.18)
    host.acn_obj_set_material(tor, b"diffuse")
    host.acn_obj_set_texture_field_chess(tor, A.v3(0.2, 0.4, 0.9), A.v3(0.9, 0.9, 0.9), 2.0)
    host.acn_obj_move(tor, A.v3(1.7, -0.6, -0.5))
    objs.append(tor)
    if extra:
        more = host.acn_obj_sphere_s_create(0.2)
        host.acn_obj_set_material(more, b"diffuse")
        host.acn_obj_move(more, A.v3(0, -2, -0.8))
        objs.append(more)
    if scaled is not None:
        inner = host.acn_obj_sphere_s_create(scaled[0])
        host.acn_obj_set_material(inner, b"diffuse")
        so = host.acn_obj_scale_s_create_scale(inner, A.v3(1.0, 1.0, 0.5))
        host.acn_obj_discard(inner)
        if scaled[1]:
            m = rotz(scaled[1])
            host.acn_obj_rotate(so, C.byref(m))
        host.acn_obj_move(so, A.v3(0.2, -2.5, -0.8))
        objs.append(so)
    for o in objs:
        sc.push(o)
        host.acn_obj_discard(o)
    flat = sc.flatten()
    if skew:
        flat = skewed(flat, ball_node(flat))
    return sc, flat


def skewed(flat, node):
    from actinon_amd.motion import copy_flat
    out = copy_flat(flat)
    out.c.nodes[node].rax[1] += 1e-6
    return out


def matter_elems(flat):
    return flat.elems_of(flat.c.matter_root)


def ball_node(flat):
    """the node of the ball: the sphere of matter whose radiance is 0 and that is textured, first in push order"""
    for i in matter_elems(flat):
        nd = flat.node(i)
        if nd.type == abi.ACN_SPHERE and nd.radiance == 0 and nd.texture >= 0:
            return i
    raise AssertionError("no ball")


# ---- the two rendered frames ----
TURN_DEG, SHIFT, ORBIT_DEG = 10.0, (0.15, 0.0, 0.0), 2.0


def copy_params(p):
    q = abi.Params()
    C.memmove(C.addressof(q), C.addressof(p), C.sizeof(abi.Params))
    return q


def two_frames():
    """the pose scene at 96 x 72; frame B has the ball turned TURN_DEG about z through its centre, shifted by SHIFT, and the camera
    orbited by ORBIT_DEG -> dict of prev_flat, cur_flat, prev_params, cur_params"""
    from actinon_amd.cameras import orbit_camera
    _, prev_flat = build_pose()
    _, cur_flat = build_pose(turn_deg=TURN_DEG, shift=SHIFT)
    prev_params = copy_params(prev_flat.params)
    cur_params = copy_params(prev_flat.params)
    for k, v in orbit_camera(prev_flat.params, ORBIT_DEG).items():
        getattr(cur_params, k)[:] = v
    return dict(prev_flat=prev_flat, cur_flat=cur_flat, prev_params=prev_params, cur_params=cur_params)


def synthetic_stats(n, seed=7):
    """statistics records of 1 .. 9 samples with random mean and m2"""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, STATS))
    st[:, 0] = rng.integers(1, 10, n)
    st[:, 1:4] = rng.uniform(0.0, 2.0, (n, 3))
    st[:, 4:7] = rng.uniform(0.0, 1.0, (n, 3))
    return st

"""numpy model of acn_project_points and acn_reproject (include/actinon_hip.h): the expressions of the header in the header's order,
vectorised over positions.  numpy's elementwise + - * / and floor are IEEE binary64 and never contracted; the camera basis is
lens_model.Camera (k_camera_setup's expressions, sqrt through the host build of csrc/acn_detmath.h: the `detmath_cpu` fixture), so the
device is compared with this model bit for bit (lens_layers_model.same_bits: which NaN a NaN is stays open).  Also the hand-made
records of the tests: a previous raster of 7 x 5 under an axis-aligned camera, in which every number is exact."""
import numpy as np

import lens_model as M
import stats_model as T
from actinon_amd import abi

KINDS_SET, HOPS_SET = 1, 2
DEFAULT_REJECT_KINDS = 4 | 8 | 16 | 64                  # CHROMATIC | FRESNEL | TRANSPARENT | CUT
DEFAULT_MAX_HOPS, DEFAULT_NORMAL_MIN, DEFAULT_PLANE_TOLERANCE, DEFAULT_MAX_HISTORY = 0, 0.9, 0.01, 32.0
SURF, STATS = 16, 8


def project(cam, P):
    """P [n,3] -> ( q [n,2] with NaN where not PROJECTED, depth [n], PROJECTED [n] ) for a lens_model.Camera"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    hh, hw = float(cam.height >> 1), float(cam.width >> 1)
    with np.errstate(all="ignore"):
        v = P - cam.position
        ly = M.dot(v, cam.V)
        s = cam.focal / ly
        qx = (M.dot(v, cam.R) * s) * hh + hw
        qy = hh - (M.dot(v, cam.T) * s) * hh
        ok = (ly > 0.0) & np.isfinite(qx) & np.isfinite(qy)
    q = np.stack([np.where(ok, qx, np.nan), np.where(ok, qy, np.nan)], axis=-1)
    return q, ly, ok


def int32(x):
    with np.errstate(invalid="ignore"):
        return x.astype(np.int32)


def reproject(lib, cur, prev_params, prev_surf, prev_stats, reject_kinds=None, max_hops=None, normal_min=None, plane_tolerance=None,
              max_history=None, detail=None):
    """-> ( stats [n,8], motion [n,2] ).  None is the default of the header.  detail (a dict) receives `hit`, `projected`, `eligible`
    [n] and `valid` [n,4]"""
    reject = DEFAULT_REJECT_KINDS if reject_kinds is None else int(reject_kinds)
    hops_max = DEFAULT_MAX_HOPS if max_hops is None else int(max_hops)
    nmin = DEFAULT_NORMAL_MIN if normal_min in (None, 0) else float(normal_min)
    tol = DEFAULT_PLANE_TOLERANCE if plane_tolerance in (None, 0) else float(plane_tolerance)
    cap = DEFAULT_MAX_HISTORY if max_history in (None, 0) else float(max_history)
    cur = np.ascontiguousarray(cur, dtype=np.float64).reshape(-1, SURF)
    W, H = int(prev_params.image_width), int(prev_params.image_height)
    ps = np.ascontiguousarray(prev_surf, dtype=np.float64).reshape(H * W, SURF)
    pt = np.ascontiguousarray(prev_stats, dtype=np.float64).reshape(H * W, STATS)
    n = len(cur)
    cam = M.Camera(lib, prev_params)
    with np.errstate(all="ignore"):
        hit = cur[:, 0] < np.inf                                              # 1
        P, N = cur[:, 1:4], cur[:, 4:7]
        q, _, ok = project(cam, P)                                            # 2
        projected = hit & ok
        motion = np.where(projected[:, None], q, np.nan)
        eligible = projected & ((int32(cur[:, 12]).astype(np.uint32) & np.uint32(reject)) == 0) & (int32(cur[:, 13]) <= hops_max)   # 3
        qx, qy = np.where(projected, q[:, 0], 0.0), np.where(projected, q[:, 1], 0.0)
        fx, fy = qx - 0.5, qy - 0.5                                           # 4
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        key = int32(cur[:, [7, 8, 13]])
        pkey = int32(ps[:, [7, 8, 13]])
        pempty = T.empty(pt)
        limit = tol * cur[:, 0]
        sw, sn, sm, s2 = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        valid = np.zeros((n, 4), dtype=bool)
        for k in range(4):
            x, y = (x0 + 1.0 if k & 1 else x0), (y0 + 1.0 if k & 2 else y0)
            w = (tx if k & 1 else 1.0 - tx) * (ty if k & 2 else 1.0 - ty)
            inside = (x >= 0.0) & (x < float(W)) & (y >= 0.0) & (y < float(H))
            p = np.where(inside, y, 0.0).astype(np.int64) * W + np.where(inside, x, 0.0).astype(np.int64)   # 5
            r, t = ps[p], pt[p]
            D = r[:, 1:4] - P
            v = (eligible & inside & (w > 0.0) & ~pempty[p] & (r[:, 0] < np.inf) & (pkey[p] == key).all(axis=1)
                 & (M.dot(N, r[:, 4:7]) >= nmin) & (np.abs(M.dot(N, D)) <= limit))
            valid[:, k] = v
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
        detail.update(hit=hit, projected=projected, eligible=eligible, valid=valid)
    return out, motion


# ---- the hand-made records ----
PW, PH = 7, 5                                                                 # the previous raster
DEPTH = 2.0                                                                   # every point lies 2 in front of the camera: s = 0.5
TOL_AT = 2.0 ** -6                                                            # a plane_tolerance whose limit, TOL_AT * DEPTH, is exact


def axis_params(width=PW, height=PH):
    """an abi.Params whose camera is the identity: position 0, view +y, top +z, focal length 1.  With the point ( a, 2, c ):
    qx = a + ( width >> 1 ), qy = ( height >> 1 ) - c, all exact (s = 1 / 2 and hh = 2 cancel at height 4 or 5)"""
    p = abi.Params()
    p.image_width, p.image_height, p.gamma = width, height, 1.0
    p.camera_view_direction[:] = (0.0, 1.0, 0.0)
    p.camera_top_direction[:] = (0.0, 0.0, 1.0)
    p.camera_focal_length = 1.0
    p.trace_depth, p.trace_min_intensity, p.direct_samples, p.path_samples, p.max_path_length = 11, 0.01, 1, 1, 100.0
    return p


def point_at(qx, qy, width=PW, height=PH):
    assert (height >> 1) == 2
    return np.array([qx - float(width >> 1), DEPTH, 2.0 - qy])


def surface_record(qx, qy, e=3, x=-1, h=0, kind=2, width=PW, height=PH):
    r = np.zeros(SURF)
    r[0] = DEPTH
    r[1:4] = point_at(qx, qy, width, height)
    r[4:7] = (0.0, -1.0, 0.0)
    r[7], r[8], r[9:12], r[12], r[13], r[14] = e, x, 0.5, kind, h, 1.0
    return r


def prev_raster(seed=5):
    """-> ( surf [35,16], stats [35,8] ) of the 7 x 5 raster: pixel ( x, y ) holds the surface point of its centre, a record of 2 .. 9
    samples with random mean and m2, and the special pixels the patterns aim at"""
    rng = np.random.default_rng(seed)
    surf = np.stack([surface_record(x + 0.5, y + 0.5) for y in range(PH) for x in range(PW)])
    st = np.zeros((PW * PH, STATS))
    st[:, 0] = 2.0 + (np.arange(PW * PH) % 8)
    st[:, 1:4] = rng.uniform(0.0, 2.0, (PW * PH, 3))
    st[:, 4:7] = rng.uniform(0.0, 1.0, (PW * PH, 3))
    at = lambda x, y: y * PW + x
    st[at(1, 1)] = 0.0                                                        # EMPTY: zeros, n below 1, a NaN n, an infinite n
    st[at(2, 1), 0] = 0.5
    st[at(5, 3), 0] = np.nan
    st[at(6, 3), 0] = np.inf
    surf[at(4, 1)] = 0.0; surf[at(4, 1), 0] = np.inf; surf[at(4, 1), 7:9] = -1.0   # a miss
    surf[at(1, 3), 7] = 4                                                     # another enter object, exit object, hops
    surf[at(2, 3), 8] = 0
    surf[at(0, 3), 13] = 1
    c = np.sqrt(1.0 - 0.81)
    surf[at(5, 1), 4:7] = (0.0, -0.9, c)                                      # dot( N, N' ) = 0.9 exactly, and one ulp below
    surf[at(6, 1), 4:7] = (0.0, -np.nextafter(0.9, 0.0), c)
    surf[at(5, 2), 2] = DEPTH + TOL_AT * DEPTH                                # | dot( N, D ) | = TOL_AT * DEPTH exactly, and one ulp above
    surf[at(6, 2), 2] = np.nextafter(DEPTH + TOL_AT * DEPTH, np.inf)
    st[at(0, 4), 0], st[at(1, 4), 0], st[at(2, 4), 0], st[at(3, 4), 0] = 1.0, 40.0, 32.0, np.nextafter(32.0, np.inf)
    st[at(4, 4), 1] = -0.0
    return surf, st


def patterns():
    """-> ( names, records [P,16] ): the current records the tests rotate over the lanes"""
    out = []
    add = lambda name, r: out.append((name, r))
    R = surface_record
    add("a pixel centre: one tap of weight 1", R(3.5, 2.5))
    add("halfway between four", R(4.0, 3.0))
    add("halfway, one EMPTY tap", R(3.0, 2.0))
    add("tx == 0", R(3.5, 2.25))
    add("ty == 0", R(3.25, 2.5))
    add("x0 == -1", R(0.25, 2.25))
    add("x0 == W' - 1", R(6.75, 0.75))
    add("y0 == -1", R(3.25, 0.25))
    add("y0 == H' - 1", R(3.25, 4.75))
    add("the corner x0 == -1, y0 == -1", R(0.25, 0.125))
    add("the corner beyond W', H'", R(6.875, 4.75))
    add("left of the image", R(-5.0, 2.5))
    add("below the image", R(3.5, 9.0))
    r = R(3.5, 2.5); r[2] = -2.0; add("behind the camera", r)
    r = R(3.5, 2.5); r[2] = 0.0; add("ly == 0", r)
    r = R(3.5, 2.5); r[2] = -0.0; add("ly == -0", r)
    r = R(3.5, 2.5); r[1] = np.nan; add("a NaN in P", r)
    r = R(3.5, 2.5); r[3] = np.inf; add("an inf in P", r)
    r = R(3.5, 2.5); r[2] = np.inf; add("an infinite depth", r)
    r = R(3.5, 2.5); r[1:4] = (1.0, 1e-300, 0.0); add("qx of 1e300", r)
    r = R(3.5, 2.5); r[1:4] = (0.0, 1e-300, -1.0); add("qy of 1e300", r)
    r = np.zeros(SURF); r[0] = np.inf; r[7:9] = -1.0; r[14] = 1.0; add("a miss", r)
    add("another enter object", R(3.5, 2.5, e=4))
    add("another exit object", R(3.5, 2.5, x=0))
    add("hops 1 on a tap of hops 0", R(3.5, 2.5, h=1))
    add("hops 1 on a tap of hops 1", R(0.5, 3.5, h=1))
    add("hops 0 on a tap of hops 1", R(0.5, 3.5))
    add("an EMPTY tap alone", R(1.5, 1.5))
    add("two EMPTY taps: all invalid", R(2.0, 1.5))
    add("EMPTY by a NaN n and by an infinite n", R(6.0, 3.5))
    add("a miss tap alone", R(4.5, 1.5))
    add("a miss tap among four", R(4.25, 1.75))
    add("enter and exit differ on both taps", R(2.0, 3.5))
    add("one tap of two matches", R(3.0, 3.5))
    add("classes differ on two of four", R(1.75, 3.75))
    add("the normal at the threshold", R(5.5, 1.5))
    add("the normal one ulp beyond", R(6.5, 1.5))
    add("the normal: one of two taps", R(6.0, 1.5))
    add("the plane at the threshold of TOL_AT", R(5.5, 2.5))
    add("the plane one ulp beyond", R(6.5, 2.5))
    add("n == 1", R(0.5, 4.5))
    add("n above max_history", R(1.5, 4.5))
    add("n at max_history", R(2.5, 4.5))
    add("n one ulp above max_history", R(3.5, 4.5))
    add("n of 1 and 40 mixed", R(1.0, 4.5))
    add("a mean of -0.0", R(4.5, 4.5))
    for kind in (1, 2, 4, 8, 16, 32, 64, 1 | 2 | 32, 2 | 8 | 16):
        add(f"kind bits {kind}", R(3.5, 2.5, kind=kind))
    rng = np.random.default_rng(11)
    for j in range(12):
        add(f"random {j}", R(float(rng.uniform(-0.5, PW + 0.5)), float(rng.uniform(-0.5, PH + 0.5))))
    names = [o[0] for o in out]
    assert len(set(names)) == len(names)
    return names, np.stack([o[1] for o in out])


# the parameter sets the hand-made records are run with: the defaults; exact thresholds, a small cap and hops allowed; every kind taken
PARAM_SETS = {
    "defaults": {},
    "exact": dict(plane_tolerance=TOL_AT, normal_min=0.875, max_history=8.0, max_hops=1, reject_kinds=1),
    "all kinds, no normal test": dict(reject_kinds=0, normal_min=-1.0, plane_tolerance=1e6, max_history=1.0),
}


def tiled(n):
    """position i is pattern i % P -> [n,16]"""
    rec = patterns()[1]
    return np.ascontiguousarray(rec[np.arange(n) % len(rec)])

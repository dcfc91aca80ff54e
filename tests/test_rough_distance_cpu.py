"""The oracle's distance objects and rough surfaces against two references that share no code with it (tests/rough_model.py):
the torus in closed form and the roughness formula in numpy.  tests/test_gpu_rough_distance.py compares the device with the
oracle bit for bit on the same scene and rays; these tests are what makes that agreement worth something.  No GPU."""
from collections import Counter

import numpy as np
import pytest

import ray_sets as R
import rough_model as M

EPS = R.F3_EPS


@pytest.fixture(scope="module")
def S(oracle):
    return R.RoughDistanceSets(oracle)


def torus_hits(S):
    """per single-torus role: ( node, rays, classes, a ) of the rough scene"""
    for role in R.TORUS_ROLES:
        rs, a, nor, ho, ta, tnor = S.sets[role]
        yield role, S.flat.node(S.elems[role]), rs, a, nor


def test_scene_layout(S):
    """the roles are what the issue names; the twin has the same nodes but for surface_roughness"""
    assert len(S.roles) == 23 and len(set(S.roles)) == 23
    for i in range(S.flat.c.n_nodes):
        a, b = S.flat.node(i), S.twin.node(i)
        assert (a.type, a.child0, a.child1, a.flags, a.cycles, a.sdf_kind) == (b.type, b.child0, b.child1, b.flags, b.cycles, b.sdf_kind)
        assert a.pos[:] == b.pos[:] and a.rax[:] == b.rax[:] and a.prm[:] == b.prm[:] and a.env_radius == b.env_radius
        assert b.surface_roughness == 0
    n = S.flat.node
    assert n(S.elems["torus"]).flags & 1 and n(S.elems["torus"]).cycles == 200 and n(S.elems["torus"]).prm[0] == 2.0
    assert not n(S.elems["torus_bare"]).flags & 1 and n(S.elems["torus_bare"]).sdf_kind == R.ACN_SDF_TORUS
    assert n(S.elems["torus_short"]).cycles == 3
    assert n(S.elems["sdf_sphere"]).prm[0] == 1 / 0.37 and not n(S.elems["sdf_sphere"]).flags & 1
    assert n(S.elems["sdf_default"]).sdf_kind == R.ACN_SDF_SPHERE and n(S.elems["sdf_default"]).prm[0] == 1.0
    assert n(S.elems["not_rough"]).surface_roughness == -0.01
    for role in ("torus_and_ball", "torus_minus_half", "torus_scaled", "torus_hole", "torus_deep"):
        assert len(R.tori_of(S.flat, S.elems[role])) == 1, role
    # different values on a parent and on its operands
    e = n(S.elems["rough_leaf_pair"])
    assert len({e.surface_roughness, n(e.child0).surface_roughness, n(e.child1).surface_roughness}) == 3
    e = n(S.elems["rough_pair_only"])
    assert e.surface_roughness > 0 and n(e.child0).surface_roughness == 0 and n(e.child1).surface_roughness == 0
    tree = S.rough_nodes("rough_tree")
    kinds = {n(k).type in (R.ACN_PAIR_INSIDE, R.ACN_PAIR_OUTSIDE) for k in tree}
    assert len(tree) >= 4 and kinds == {True, False}, tree   # leaves and pairs
    # (a pair takes the properties of its first operand: pairs above a rough first operand are rough as well)
    poly = S.rough_nodes("rough_polytope")
    assert S.elems["rough_polytope"] in poly and sum(n(k).type == R.ACN_PLANE for k in poly) == 8   # the composite and 8 of 24 planes
    assert len(S.rough_nodes("rough_compound")) == 32       # every second of 64 spheres
    assert len(R.leaves_of(S.flat, S.elems["rough_compound"])) == 64
    for role, (rs, *_) in S.sets.items():
        assert len(rs) <= 1700, (role, len(rs))


def test_exact_surface(S):
    """every finite hit a of a torus: the point at a + f3_eps lies within f3_eps / inv_scale (+ 1e-12) of the exact torus --
    the loop's exit test | dist | <= f3_eps in local units.  Measured on these rays: 5.000000006e-7 at inv_scale 2 (bound
    5.00001e-7).  Hit points on the torus' axis are left out (rough_model.on_torus_axis)."""
    worst = 0.0
    for role, node, rs, a, nor in torus_hits(S):
        fin = np.isfinite(a)
        fin[fin] = ~M.on_torus_axis(node, R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], a[fin] + EPS))
        assert fin.sum() >= 10, role
        p = R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], a[fin] + EPS)
        res = np.abs(M.exact_torus_sdf(node, p))
        bound = EPS / node.prm[0] + 1e-12
        worst = max(worst, float(res.max()))
        assert (res <= bound).all(), f"{role}: {int((res > bound).sum())} hits off the exact torus, worst {float(res.max())}, classes {Counter(rs.cls[fin][res > bound])}"
    print("exact surface: largest residual", worst)


def test_normal(S):
    """the finite-difference normal against the exact one: per component within 2 f3_eps / ( 2 prm[1] ) -- the forward
    difference's truncation h / 2 rho at the smallest radius of curvature rho = prm[1] (local units, h = f3_eps), the factor 2
    for rounding.  Measured on these rays 1.551e-6 against the derived 1.389e-6 (bound 2.78e-6); a transposed rax or a wrong
    axis is off by 0.1 or more.  rough_torus is taken from the smooth twin (the same node without its roughness)."""
    worst = 0.0
    for role in R.TORUS_ROLES:
        rs, a, nor, ho, ta, tnor = S.sets[role]
        node = S.flat.node(S.elems[role])
        fin = np.isfinite(ta)
        fin[fin] = ~M.on_torus_axis(node, R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], ta[fin] + EPS))
        p = R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], ta[fin] + EPS)
        err = np.abs(tnor[fin] - M.exact_torus_normal(node, p)).max(axis=1).astype(np.float64)
        bound = 2 * EPS / (2 * node.prm[1])
        worst = max(worst, float(err.max()))
        assert (err <= bound).all(), f"{role}: normal off by {float(err.max())} (bound {bound}), classes {Counter(rs.cls[fin][err > bound])}"
    print("normal: largest error of a component", worst)


def outside_origin(node, rays):
    """origins outside the exact torus, but for those on its axis (rough_model.on_torus_axis: the reference's function calls
    the axis near the centre inside)"""
    return np.asarray(M.exact_torus_sdf(node, rays[:, :3]) > 0) & ~M.on_torus_axis(node, rays[:, :3])


def test_axis_function(S, oracle):
    """what the reference's torus function does on the axis (f == 0: | z | - prm[1], distance.c:88): torus_bare is not rotated,
    so points of its axis have local x = y = 0 exactly -- the oracle calls them inside where | z | < prm[1] / inv_scale although
    the torus is nowhere near; one ulp off the axis the torus is back.  (A ray along the axis lands exactly f3_eps behind that
    phantom surface, where | dist | <= f3_eps is decided by the rounding of the last step: hit or miss, the device has to agree.)"""
    e = S.elems["torus_bare"]
    node = S.flat.node(e)
    assert R.rax(node).tolist() == np.eye(3).tolist()
    c, r = np.array(node.pos[:]), node.prm[1] / node.prm[0]
    z = np.array([-2.0, -1.01, -0.99, -0.5, 0.0, 0.5, 0.99, 1.01, 2.0]) * r
    pts = c + np.outer(z, [0, 0, 1.0])
    assert (oracle.obj_sides(S.flat, e, pts) == np.where(np.abs(z) < r, -1, 1)).all()
    off = pts + np.array([np.spacing(c[0]), 0, 0])
    assert (M.exact_torus_sdf(node, off) > 0).all() and (oracle.obj_sides(S.flat, e, off) == 1).all()


def sdf_along(node, rays, t):
    """exact_torus_sdf at ray parameters t [n, m] -> [n, m]"""
    p = rays[:, None, :3] + rays[:, None, 3:] * t[:, :, None]
    return M.exact_torus_sdf(node, p.reshape(-1, 3)).reshape(t.shape)


def test_no_early_root(S):
    """hits from outside origins: the exact function stays positive on [ 0, a - 2 f3_eps ] (2000 samples per ray): the march
    never steps over a crossing.  Measured minimum on these rays: 2.9e-17, at the origin of a tangent ray that starts on the
    surface (k = 0); above 0."""
    lowest = np.inf
    for role, node, rs, a, nor in torus_hits(S):
        use = np.isfinite(a) & (a > 2 * EPS) & outside_origin(node, rs.rays)
        t = np.linspace(0, 1, 2000)[None, :] * (a[use] - 2 * EPS)[:, None]
        low = sdf_along(node, rs.rays[use], t).min(axis=1)
        lowest = min(lowest, float(low.min()))
        assert (low > 0).all(), f"{role}: {int((low <= 0).sum())} hits lie behind a crossing of the exact torus, classes {Counter(rs.cls[use][low <= 0])}"
    print("no early root: smallest exact distance before a hit", lowest)


def deepest_miss(node, rays, cls=None):
    """per ray: how deep below the exact torus' surface the ray gets (0: it stays outside) -- 1200 samples along the ray up to
    past the torus, then three refinements about the lowest one"""
    c = np.array(node.pos[:])
    span = np.linalg.norm(rays[:, :3] - c, axis=1) + 2.0 / node.prm[0]
    out = np.zeros(len(rays))
    # a coarse pass (spacing < 4e-3: the function is 1-Lipschitz, so a ray that goes below 0 shows a sample below 0.01)
    t = np.linspace(0, 1, 1200)[None, :] * span[:, None]
    f = sdf_along(node, rays, t)
    near = np.flatnonzero(f.min(axis=1) < 0.01)
    k = f[near].argmin(axis=1)
    low = f[near].min(axis=1).astype(np.float64)
    step = span[near] / 1199
    tk = t[near, k]
    for rnd in range(3):
        lo, hi = np.maximum(tk - step, 0), tk + step
        t2 = lo[:, None] + np.linspace(0, 1, 200)[None, :] * (hi - lo)[:, None]
        f2 = sdf_along(node, rays[near], t2).astype(np.float64)
        low = np.minimum(low, f2.min(axis=1))
        tk, step = t2[np.arange(len(near)), f2.argmin(axis=1)], (hi - lo) / 199
    out[near] = np.maximum(0.0, -low)
    return out


# the deepest exact penetration of a ray the oracle reports as a miss: cycles = 200, 6000 uniform rays of the seed below, outside
# origins -- all of them grazing rays.  A whole missed crossing is as deep as the tube's radius, 0.18.
DEEPEST_MISS = 1.684e-4   # measured: torus 1.239e-5, torus_bare 0, rough_torus 1.684e-4


def test_misses(S, oracle):
    """the oracle's misses with cycles = 200, uniform rays: none crosses the exact torus deeper than 4 x DEEPEST_MISS.
    The aimed classes are reported, not bounded -- the march of the reference has two ways to lose a deep crossing, and they find
    both: a ray that grazes the tube first (torus_tangent on the inner side) spends its 200 cycles creeping along the tangent
    point, f3_eps at a time, and never reaches the crossing behind it; a ray that meets the surface head on (torus_axis through
    the tube's centre circle, secondary rays along the normal) lands exactly f3_eps inside, where | dist | <= f3_eps is decided
    by the rounding of the last step.  The device has to reproduce every one of them (tests/test_gpu_rough_distance.py)."""
    for role in ("torus", "torus_bare", "rough_torus"):
        e = S.elems[role]
        node = S.flat.node(e)
        c, rad = np.array(node.pos[:]), 1.01 * (1 + node.prm[1]) / node.prm[0]
        rays = R.uniform(np.random.default_rng(21), c, rad, 6000).rays
        a, _ = oracle.obj_ray_hits(S.flat, e, rays)
        use = ~np.isfinite(a) & outside_origin(node, rays)
        assert use.sum() >= 1000
        # (a line that stays outside the torus' bounding ball cannot cross it)
        foot = (rays[:, :3] - c) - rays[:, 3:] * ((rays[:, :3] - c) * rays[:, 3:]).sum(axis=1)[:, None]
        use &= np.linalg.norm(foot, axis=1) < rad
        depth = deepest_miss(node, rays[use])
        print(f"misses of {role}: {int(use.sum())} of 6000 uniform rays pass the bounding ball, deepest penetration {depth.max():.3e}")
        assert (depth <= 4 * DEEPEST_MISS).all(), f"{role}: a miss crosses the torus {depth.max()} deep: ray {rays[use][depth.argmax()].tolist()}"
        rs, a, *_ = S.sets[role]
        use = ~np.isfinite(a) & outside_origin(node, rs.rays)
        depth = deepest_miss(node, rs.rays[use])
        print(f"   aimed rays of {role}: deepest penetration of a miss by class",
              {k: float(f"{depth[rs.cls[use] == k].max():.3e}") for k in sorted(set(rs.cls[use]))})


def test_short_cycles_miss_more(S, oracle):
    """cycles = 3 ends most rays through the cycle count: on the SAME rays torus_short (moved onto torus' place: the two
    differ in position and rotation) has fewer hits than torus.  Measured: 327 hits against 746 of 1538 rays."""
    rs, a, *_ = S.sets["torus"]
    ts, tl = S.flat.node(S.elems["torus_short"]), S.flat.node(S.elems["torus"])
    # the same rays in torus_short's frame: local coordinates kept, world = pos_s + rax_s^T rax_l ( p - pos_l )
    T = R.rax(ts).T @ R.rax(tl)
    rays = np.concatenate([(rs.rays[:, :3] - np.array(tl.pos[:])) @ T.T + np.array(ts.pos[:]), rs.rays[:, 3:] @ T.T], axis=1)
    rays[:, 3:] = R.unit(rays[:, 3:])
    b, _ = oracle.obj_ray_hits(S.flat, S.elems["torus_short"], rays)
    h_long, h_short = int(np.isfinite(a).sum()), int(np.isfinite(b).sum())
    print(f"hits of {len(rays)} rays: cycles 200: {h_long}, cycles 3: {h_short}")
    assert h_short < h_long and h_short >= 10


def test_twin(S):
    """rough scene against smooth twin: the same distance bits on every element; | |nor| - 1 | <= 4e-16 ... of a rescaled
    normal; where the hit's path holds a rough node the normal differs; not_rough's normals are the twin's"""
    for role, (rs, a, nor, ho, ta, tnor) in S.sets.items():
        assert (M.bits(a) == M.bits(ta)).all(), f"{role}: roughness moved a distance"
        fin = np.isfinite(a)
        ln = np.sqrt((nor[fin].astype(np.longdouble) ** 2).sum(axis=1))
        assert (np.abs(ln - 1) <= 1e-8).all(), role            # v_of_length leaves | r^2 - 1 | < 1e-8 alone
        diff = fin & (M.bits(nor) != M.bits(tnor)).any(axis=1)
        rescaled = diff & (np.abs((nor ** 2).sum(axis=1) - 1) > 1e-12)
        if S.rough_nodes(role):
            # a roughened normal was brought to length 1 by one multiplication per component: 4e-16
            assert (np.abs(np.sqrt((nor[diff].astype(np.longdouble) ** 2).sum(axis=1)) - 1) <= 4e-16).all(), role
            assert diff.sum() >= 100, (role, int(diff.sum()))
        else:
            assert not diff.any(), f"{role}: no rough node, but {int(diff.sum())} normals differ from the twin's"
    rs, a, nor, ho, ta, tnor = S.sets["not_rough"]
    assert (M.bits(nor) == M.bits(tnor)).all() and np.isfinite(a).sum() >= 100


def test_roughness_model(S, oracle, detmath_cpu):
    """the oracle's rough normals equal rough_model.roughen applied node by node (check_rough_steps: operand first, parent
    last; under a scale wrapper the operand is seeded by the hit position in the SCALED frame, objects.c:1418-1437 hands the
    operand the transformed ray and objects.c:261-284 seeds with that ray), bit for bit, on every non-compound element"""
    hits = lambda node, rays: oracle.obj_ray_hits(S.flat, node, rays)       # noqa: E731
    twin = lambda node, rays: oracle.obj_ray_hits(S.twin, node, rays)       # noqa: E731
    sides = lambda node, pts: oracle.obj_sides(S.flat, node, pts)           # noqa: E731
    total = Counter()
    for role, e in S.elems.items():
        if S.flat.node(e).type == R.ACN_COMPOUND:
            continue
        stats = {}
        bad = M.check_rough_steps(S.flat, S.twin, e, S.sets[role][0].rays, hits, twin, sides, oracle, detmath_cpu, stats)
        print("model", role, stats)
        assert bad == 0, f"{role}: {bad} normals differ from the model; first {stats.get('first_bad')}"
        if S.rough_nodes(role):
            assert sum(v for k, v in stats.items() if k.startswith("rough_")) >= 100, (role, stats)
        total.update({k: v for k, v in stats.items() if k != "first_bad"})
    print("model, all roles:", dict(total))
    for k in ("rough_leaf", "rough_pair", "rough_neg", "rough_scale", "smooth_pair"):
        assert total[k] >= 50 or k == "rough_scale", (k, total)
    # the simple compound: the hit sphere's own step
    rs, a, nor, ho, ta, tnor = S.sets["rough_compound"]
    fin = np.isfinite(a)
    r = np.array([S.flat.node(int(k)).surface_roughness if k >= 0 else 0.0 for k in ho])
    want = tnor.copy()
    for v in set(r[fin & (r > 0)]):
        m = fin & (r == v)
        # the twin's winner of a tie is the same table entry: the same leaf, smooth
        want[m] = M.roughen(tnor[m], R.ray_pos(rs.rays[m, :3], rs.rays[m, 3:], a[m]), float(v), oracle, detmath_cpu)
    assert (M.bits(want[fin]) == M.bits(nor[fin])).all()
    assert (fin & (r > 0)).sum() >= 100 and (fin & (r == 0)).sum() >= 100


def test_not_vacuous(S, oracle):
    """the scene alone meets the counts the device test asserts on the device's answers.  Measured (rays / finite hits): torus
    1538 / 746 (tangent rays 66 hits, 94 misses; inside 120 hits), torus_bare 1082 / 345 (62, 98; 120; 737 misses), torus_short
    1142 / 140, sdf_sphere 940 / 476, sdf_default 940 / 470, torus_and_ball 1338 / 255, torus_minus_half 1566 / 545, torus_scaled
    1092 / 418, torus_hole 1518 / 678, torus_deep 1478 / 416, rough_sphere 940 / 562, rough_plane 940 / 501, rough_ellipsoid
    910 / 395, rough_cone 940 / 610, rough_torus 1538 / 733 (61, 99; 120), rough_leaf_pair 832 / 320, rough_pair_only 880 / 355,
    rough_neg 874 / 361 (110 on the rough wall), rough_scaled 940 / 432, rough_tree 1016 / 466, rough_polytope 868 / 355,
    rough_compound 1100 / 396 (226 on a rough sphere), not_rough 940 / 582; 3181 of 6726 scene rays end on a rough or distance
    element."""
    S.check_counts(S.counts())
    # hard answers of the scene-level queries need the device; what the oracle can say: trans hits on a rough or distance element
    rs = R.rough_distance_scene_rays(np.random.default_rng(3), oracle, S.flat)
    ta, tn, tex, ten = oracle.trans_hits(S.flat, S.root, rs.rays)
    special = {S.elems[r] for r in S.roles if S.rough_nodes(r) or R.tori_of(S.flat, S.elems[r]) or r.startswith("sdf")}
    n = int((np.isfinite(ta) & np.isin(tex, list(special))).sum())
    print("trans hits on a rough or distance element:", n, "of", len(rs))
    assert n >= 100

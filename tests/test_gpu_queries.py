"""The device's traversal shortcuts, query by query and ray by ray, against the CPU oracle (run on the MI355X: -m gpu).

The image tests compare whole frames; the shortcuts of acn_device.h (envelope pre-tests, interval-prune programs, the
culled and reversed simple-compound tables, cone culling, the any-hit and fast forms of the root loops, the lock-step
machines) each claim to leave results unchanged, and the rays where their margins matter are rare in an image.  Here the
test seam acn_query_rays runs each shortcut on ray sets aimed at those margins (tests/ray_sets.py) and every answer is
checked against the oracle's one-ray functions (acn_oracle_query_rays).  A failure names the query, the element and the
ray class."""
from collections import Counter

import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
from query_checks import MACHINE_TYPES, VARIANTS, bits, check_trans_and_occlusion, report_mismatch, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def qscene():
    sc, roles = R.query_scene(seed=1)
    flat = sc.flatten()
    handles = {"default": upload(flat), "prune_min_1": upload(flat, ACN_PRUNE_MIN=1)}
    for h in handles.values():
        assert h.query_rays("elements", flat.c.matter_root, n=1)[0, 3] == 0   # nodes in global memory (see VARIANTS)
    yield sc, flat, roles, handles
    for h in handles.values():
        h.close()


def element_rays(rng, oracle, flat, e, n=1500):
    """every ray class that applies to root element e, with the oracle's hits of the uniform class"""
    node = flat.node(e)
    c, rad = R.node_ball(flat, e)
    if node.type not in (R.ACN_SPHERE,) and not (node.flags & 1):
        est = oracle.estimate_envelope(flat, e, samples=2000)
        if np.all(np.isfinite(est)) and 0 < est[3] < 10:
            c, rad = np.array(est[:3]), est[3]
    rs = R.uniform(rng, c, rad, n)
    a, nor = oracle.obj_ray_hits(flat, e, rs.rays)
    rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=200))
    rs.extend(R.tangent_ball(rng, c, rad, 60))
    rs.extend(R.far(rng, c, rad, 300))
    for ec, er in R.envelopes_of(flat, e)[:6]:
        rs.extend(R.envelope_boundary(rng, ec, er, 60))
        rs.extend(R.tangent_ball(rng, ec, er, 30))
    for leaf in R.leaves_of(flat, e)[:12]:
        ln = flat.node(leaf)
        if ln.type == R.ACN_SPHERE:
            rs.extend(R.tangent_ball(rng, np.array(ln.pos[:]), float(ln.prm[0]), 20))
        elif ln.type == R.ACN_SQUAROID:
            rays, _ = R.squaroid_tangent_lines(ln, rng, 12, digits=30)
            rs.add(rays, "tangent")
            rs.extend(R.degenerate(rng, ln, 20))
        elif ln.type == R.ACN_PLANE:
            rs.extend(R.plane_parallel(rng, ln, 20))
    return rs


@pytest.fixture(scope="module")
def element_sets(qscene, oracle):
    sc, flat, roles, handles = qscene
    rng = np.random.default_rng(11)
    out = {}
    for role, e in zip(roles, flat.elems_of(flat.c.matter_root)):
        if flat.node(e).type == R.ACN_COMPOUND:
            continue
        rs = element_rays(rng, oracle, flat, e)
        a, nor = oracle.obj_ray_hits(flat, e, rs.rays)
        out[(role, e)] = (rs, a, nor)
    return out


# ---- 1. exact hits ------------------------------------------------------------------------------------------------

def test_hits_bit_identical(qscene, element_sets):
    """HIT_LANE, HIT_UNI and ELEMENT_HIT, both scene types (nodes in global memory): the oracle's obj_ray_hit bit for
    bit (distance; normal wherever the distance is finite; the hit object of element_hit is the element)."""
    sc, flat, roles, handles = qscene
    h = handles["default"]
    for (role, e), (rs, a, nor) in element_sets.items():
        fin = np.isfinite(a)
        for lds, prune in VARIANTS:
            for op in ("hit_lane", "hit_uni", "element_hit"):
                g = h.query_rays(op, e, rs.rays, lds=lds, prune=prune)
                bad = bits(g[:, 0]) != bits(a)
                bad |= fin & (bits(g[:, 1:4]) != bits(nor)).any(axis=1)
                if op == "element_hit":
                    bad |= g[:, 4] != e
                assert not bad.any(), report_mismatch(f"{op} lds={lds} prune={prune}", role, rs, bad)


# ---- 2. sides -----------------------------------------------------------------------------------------------------

def test_sides_equal_oracle(qscene, element_sets, oracle):
    """SIDE_LANE and SIDE_UNI equal the oracle's obj_side at the ray origins and at reported hit points +- f3_eps"""
    sc, flat, roles, handles = qscene
    h = handles["default"]
    for (role, e), (rs, a, nor) in element_sets.items():
        fin = np.isfinite(a)
        pts = [rs.rays[:, :3]]
        for off in (-R.F3_EPS, R.F3_EPS):
            pts.append(R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], a[fin] + off))
        pts = np.concatenate(pts)
        want = oracle.obj_sides(flat, e, pts)
        q = np.concatenate([pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1))], axis=1)
        for lds, prune in VARIANTS:
            for op in ("side_lane", "side_uni"):
                g = h.query_rays(op, e, q, lds=lds, prune=prune)[:, 0]
                bad = g != want
                assert not bad.any(), f"{op} lds={lds} prune={prune} on {role}: {int(bad.sum())} of {len(pts)} points, first {pts[np.flatnonzero(bad)[0]].tolist()}"


# ---- 3. prune soundness -------------------------------------------------------------------------------------------

def test_prune_soundness(qscene, element_sets, oracle):
    """A skip of surely_outside or prune_run( inf ) means the oracle returns f3_inf for the element and obj_side is +1
    at the points of the ray the secondary rays would start from; prune_run( limit ) skips only beyond the limit.
    Not vacuous: skips are counted per element, and among them the rays whose line crosses a leaf of the object."""
    sc, flat, roles, handles = qscene
    rng = np.random.default_rng(5)
    totals = Counter()
    for hname, h in handles.items():
        for (role, e), (rs, a, nor) in element_sets.items():
            if flat.node(e).type not in MACHINE_TYPES:
                continue
            idx, lim = R.occlusion_limits(a, rng)
            for lds, prune in VARIANTS[:2]:
                g = h.query_rays("prune", e, rs.rays, limits=np.full(len(rs), np.inf), lds=lds, prune=prune)
                skip = (g[:, 0] != 0) | (g[:, 2] != 0)
                bad = skip & np.isfinite(a)
                assert not bad.any(), report_mismatch(f"prune ({hname}, lds={lds}, prune={prune}) skipped a hit", role, rs, bad)
                # surely_outside's skips: obj_side +1 along the ray, at points beyond the origin (the secondary class's
                # distances f3_eps and 2 f3_eps, and random ones).  (t = 0 is left out: an origin exactly on an envelope
                # sphere, moving outward, misses the envelope as a ray while obj_side counts the point itself as inside the
                # closed ball.)  prune_run decides on the hit interval H alone, which is what a = inf above checks: the
                # object's side can be -1 on a ray without a hit where an envelope clips it (objects.c:368).
                sk = np.flatnonzero(skip)
                so = np.flatnonzero(g[:, 0] != 0)
                if len(so):
                    t = np.concatenate([rng.uniform(0, 6, len(so)), np.full(len(so), R.F3_EPS), np.full(len(so), 2 * R.F3_EPS)])
                    rr = np.tile(rs.rays[so], (3, 1))
                    sides = oracle.obj_sides(flat, e, R.ray_pos(rr[:, :3], rr[:, 3:], t))
                    badp = sides != 1
                    assert not badp.any(), f"prune skipped a ray with an inside point on {role}: ray {rr[np.flatnonzero(badp)[0]].tolist()} t {t[np.flatnonzero(badp)[0]]}"
                # prune_run( limit )
                gl = h.query_rays("prune", e, rs.rays[idx], limits=lim, lds=lds, prune=prune)
                badl = (gl[:, 1] != 0) & np.isfinite(a[idx]) & (a[idx] <= lim)   # a skip claims: no hit at t <= limit
                assert not badl.any(), f"prune_run( limit ) ({hname}) on {role}: skipped {int(badl.sum())} rays with a hit at <= limit, classes {Counter(rs.cls[idx][badl])}"
                if prune:
                    crossed = 0
                    if len(sk):
                        for leaf in R.leaves_of(flat, e):
                            la, _ = oracle.obj_ray_hits(flat, leaf, rs.rays[sk])
                            crossed += int(np.isfinite(la).sum())
                    key = (hname, role, e)
                    totals[key + ("skips",)] += int(skip.sum())
                    totals[key + ("program_skips",)] += int((g[:, 2] != 0).sum())
                    totals[key + ("leaf_crossed",)] += crossed
                    totals[key + ("has_program",)] = int(g[0, 3])
                    for c, k in Counter(rs.cls[skip]).items():
                        totals[("class", hname, c)] += k
    for k in sorted(totals, key=str):
        print("prune", k, totals[k])
    for hname in handles:
        skips = sum(v for k, v in totals.items() if k[0] == hname and k[-1] == "skips")
        crossed = sum(v for k, v in totals.items() if k[0] == hname and k[-1] == "leaf_crossed")
        assert skips > 1000 and crossed > 100, (hname, skips, crossed)
    # per object group: every pair element (the types the pre-tests can rule out; complements and scale wrappers at the
    # root are never pruned) skips rays, and with ACN_PRUNE_MIN=1 its program does
    for (role, e), _ in element_sets.items():
        if flat.node(e).type in (R.ACN_PAIR_INSIDE, R.ACN_PAIR_OUTSIDE):
            assert totals[("prune_min_1", role, e, "program_skips")] >= 20, (role, e)
            assert totals[("default", role, e, "skips")] + totals[("prune_min_1", role, e, "skips")] >= 20, (role, e)
    # every CSG element gets a program with ACN_PRUNE_MIN=1, and programs skip rays there
    progs = [k for k, v in totals.items() if k[0] == "prune_min_1" and k[-1] == "has_program" and v]
    assert len(progs) >= 5
    assert sum(v for k, v in totals.items() if k[0] == "prune_min_1" and k[-1] == "program_skips") > 500


def quadric_roots(node, ray, digits=50):
    """the exact ray parameters at which the rounded ray meets the squaroid a x^2 + b y^2 + c z^2 + r = 0 (mpmath)"""
    import mpmath as mp
    mp.mp.dps = digits
    M = mp.matrix(R.rax(node).tolist())
    pos = mp.matrix([float(v) for v in node.pos[:]])
    a, b, c, r = (mp.mpf(float(v)) for v in node.prm[:4])
    p = M * (mp.matrix([mp.mpf(float(v)) for v in ray[:3]]) - pos)
    d = M * mp.matrix([mp.mpf(float(v)) for v in ray[3:]])
    A = a * d[0] ** 2 + b * d[1] ** 2 + c * d[2] ** 2
    B = a * p[0] * d[0] + b * p[1] * d[1] + c * p[2] * d[2]
    C = a * p[0] ** 2 + b * p[1] ** 2 + c * p[2] ** 2 + r
    if A == 0:
        return [float(-C / (2 * B))] if B != 0 else []
    disc = B * B - A * C
    if disc < 0:
        return []
    sq = mp.sqrt(disc)
    return [float((-B - sq) / A), float((-B + sq) / A)]


# ---- 4. interval containment --------------------------------------------------------------------------------------

def test_leaf_intervals_contain_hits(qscene, element_sets, oracle):
    """every finite oracle hit of a leaf lies in its LEAF_IV interval (iv_ball / iv_squaroid / iv_halfspace); the rays
    are those of every element the leaf belongs to, tangent and degenerate classes included"""
    sc, flat, roles, handles = qscene
    h = handles["prune_min_1"]
    slack = {}
    for (role, e), (rs, a, nor) in element_sets.items():
        for leaf in R.leaves_of(flat, e):
            la, _ = oracle.obj_ray_hits(flat, leaf, rs.rays)
            fin = np.isfinite(la)
            if not fin.any():
                continue
            g = h.query_rays("leaf_iv", leaf, rs.rays[fin])
            lo, hi = g[:, 0], g[:, 1]
            bad = ~((lo <= la[fin]) & (la[fin] <= hi))
            sub = R.RaySet(rs.rays[fin], rs.cls[fin])
            assert not bad.any(), report_mismatch(f"leaf_iv of leaf {leaf} (type {flat.node(leaf).type})", role, sub, bad)
            for c in set(sub.cls):
                m = sub.cls == c
                s = float(np.min(np.minimum(la[fin][m] - lo[m], hi[m] - la[fin][m])))
                slack[c] = min(slack.get(c, np.inf), s)
    # classes (c) and (d) against the exact geometry: the tangent point of a quadric's tangent line, computed in mpmath,
    # lies at ray parameter t* (exact, for the rounded ray); iv_squaroid's interval holds t* and t* - f3_eps (where the
    # hit is reported); degenerate rays along an axis or through an apex are the early-out (no statement: the whole ray)
    import mpmath as mp
    rng = np.random.default_rng(13)
    exact, exact_deg = [], 0
    for leaf in sorted({l for (role, e) in element_sets for l in R.leaves_of(flat, e) if flat.node(l).type == R.ACN_SQUAROID}):
        ln = flat.node(leaf)
        rays, pts = R.squaroid_tangent_lines(ln, rng, 8)
        if not len(rays):
            continue
        mp.mp.dps = 50
        ts = []
        for ray, P in zip(rays, pts):
            o = [mp.mpf(float(v)) for v in ray[:3]]
            d = [mp.mpf(float(v)) for v in ray[3:]]
            ts.append(float(mp.fsum((P[i] - o[i]) * d[i] for i in range(3)) / mp.fsum(x * x for x in d)))
        ts = np.array(ts)
        g = h.query_rays("leaf_iv", leaf, rays)
        for t in (ts, ts - R.F3_EPS):
            inside = (g[:, 0] <= t) & (t <= g[:, 1])
            assert inside.all(), f"leaf_iv of leaf {leaf}: the exact tangent point t* = {t[~inside][0]} lies outside [{g[~inside][0, 0]}, {g[~inside][0, 1]}]"
        exact.append(float(np.min(np.minimum(ts - R.F3_EPS - g[:, 0], g[:, 1] - ts))))
        dg = R.degenerate(rng, ln, 10)
        gd = h.query_rays("leaf_iv", leaf, dg.rays)
        for k, ray in enumerate(dg.rays):   # every exact crossing ahead of the origin, and f3_eps before it
            for t in quadric_roots(ln, ray):
                # up to 1e6 (the far class's range).  Beyond, a ray along a cylinder's or hyperboloid's axis meets the
                # surface only through the rounding residue of its rotated direction (A ~ 1e-32): the exact crossing (1e16
                # and more) and the one the reference's fp64 expressions report differ by tens of percent, and the
                # contract of the interval is the reported hit, checked against the oracle above for these rays too
                if 0 <= t <= 1e6:
                    exact_deg += 1
                    assert gd[k, 0] <= t - R.F3_EPS and t <= gd[k, 1], f"leaf_iv of leaf {leaf}: degenerate ray {ray.tolist()} crosses at {t} outside [{gd[k, 0]}, {gd[k, 1]}]"
    slack["tangent_exact"] = min(exact)
    assert exact_deg > 50, exact_deg
    print("smallest slack of a hit inside its leaf interval, by class:", slack)
    assert {"uniform", "secondary", "tangent"} <= set(slack)


# ---- 5. scene queries ---------------------------------------------------------------------------------------------

def scene_rays(rng, oracle, flat, n=3000):
    c = np.zeros(3)
    rs = R.uniform(rng, c, 5.0, n)
    a, nor, ho = oracle.compound_ray_hits(flat, flat.c.matter_root, rs.rays)
    rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=300))
    for e in flat.elems_of(flat.c.matter_root):
        ec, er = R.node_ball(flat, e, default_r=1.0)
        rs.extend(R.tangent_ball(rng, ec, er, 8))
    rs.extend(R.far(rng, c, 4.0, 500))
    return rs


@pytest.fixture(scope="module")
def scene_sets(qscene, oracle):
    sc, flat, roles, handles = qscene
    rs = scene_rays(np.random.default_rng(3), oracle, flat)
    a, nor, ho = oracle.compound_ray_hits(flat, flat.c.matter_root, rs.rays)
    return rs, a


def test_trans_and_occlusion(qscene, scene_sets, oracle):
    """TRANS (root_trans_hit, and root_trans_hit_fast with the hard redo) equals the oracle's compound_s_ray_trans_hit;
    root_occluded and root_occluded_fast equal compound_s_ray_hit( matter ) <= limit, and the fast form answers 2 (hard)
    only where a machine element of the root was not ruled out"""
    sc, flat, roles, handles = qscene
    rs, a = scene_sets
    counts, queries = check_trans_and_occlusion(flat, handles, rs, a, oracle)
    print("scene queries:", dict(counts), "rays", len(rs), "occlusion queries", queries)
    assert all(v > 0 for k, v in counts.items() if k[0] == "occluded_hard")


# ---- 6. cone culling ----------------------------------------------------------------------------------------------

def cone_check(h, flat, oracle, pts, lines, rng, n_random=12):
    """root_cone_cull from every point of `pts` towards the light; each point's rays are drawn in the DEVICE's frame
    (the axis and cap height CONE_CULL returns): the rim u = 1 at 16 angles, the axis, random cap directions, and for
    lines[k] (a unit vector or None) the rim direction towards that line turned by 0, +-1e-16, +-1e-15, +-1e-13 about
    the axis, and the line itself.  Every element a mask skips must be missed by every ray of its point, per the oracle;
    root_occluded_fast with the masks must equal the oracle's occlusion test.  Returns counts."""
    root = flat.c.matter_root
    els = flat.elems_of(root)[:64]
    light = flat.elems_of(flat.c.light_root)[0]
    g = h.query_rays("cone_cull", light, np.concatenate([pts, np.tile([0, 0, 1.0], (len(pts), 1))], axis=1))
    masks = g[:, 0].copy().view(np.uint64)
    counts = Counter()
    rays_of, skip_of = [], []
    for k, p in enumerate(pts):
        axis, cyl = g[k, 1:4], g[k, 5]
        if not (g[k, 4] > 1e-6):
            continue   # a half space or more: root_cone_cull makes no statement
        x = R.unit(np.cross(axis, [0.3, 0.5, 0.8] if abs(axis[2]) > 0.9 else [0, 0, 1.0]))
        y = np.cross(axis, x)
        u = np.concatenate([np.ones(16), [0.0], rng.random(n_random)])
        phi = np.concatenate([np.linspace(0, 2 * np.pi, 16, endpoint=False), [0.0], 2 * np.pi * rng.random(n_random)])
        z = 1.0 - u * cyl
        sc_ = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        d = np.outer(sc_ * np.sin(phi), x) + np.outer(sc_ * np.cos(phi), y) + np.outer(z, axis)
        d = R.unit(d)
        if lines[k] is not None:
            d = np.concatenate([d, R.cone_frame_dirs(axis, cyl, lines[k], (0.0, 1e-16, -1e-16, 1e-15, -1e-15, 1e-13, -1e-13)),
                                [lines[k]]])
        rays = np.concatenate([np.tile(p, (len(d), 1)), d], axis=1)
        rays_of.append(rays); skip_of += [int(masks[k])] * len(rays)
        m = int(masks[k])
        for i, e in enumerate(els):
            ea = (oracle.compound_ray_hits(flat, e, rays)[0] if flat.node(e).type == R.ACN_COMPOUND
                  else oracle.obj_ray_hits(flat, e, rays)[0])
            hit = np.isfinite(ea)
            if lines[k] is not None:
                counts["rim_hits"] += int(hit[-8:].sum())
            if not (m >> i) & 1:
                continue
            counts["culled"] += 1
            assert not hit.any(), (f"root_cone_cull skipped element {i} (node {e}) from point {p.tolist()}, but a ray of the "
                                   f"cone hits it: {rays[np.flatnonzero(hit)[0]].tolist()}")
    rays = np.concatenate(rays_of)
    skip = np.array(skip_of, dtype=np.uint64)
    la, _ = oracle.obj_ray_hits(flat, light, rays)
    ok = np.isfinite(la)
    rays, skip, la = rays[ok], skip[ok], la[ok]
    ca, _, _ = oracle.compound_ray_hits(flat, root, rays)
    want = ca <= la
    for lds, prune in VARIANTS[:2]:
        o = h.query_rays("occluded", root, rays, limits=la, skip=skip, lds=lds, prune=prune)[:, 1]
        bad = ((o == 0) & want) | ((o == 1) & ~want)
        assert not bad.any(), f"root_occluded_fast with cone-cull skips: {int(bad.sum())} of {len(rays)} rays wrong, first {rays[np.flatnonzero(bad)[0]].tolist()}"
    counts["points"] += len(rays_of)
    counts["rays"] += len(rays)
    return counts


def test_cone_cull(qscene, scene_sets, oracle):
    """every element root_cone_cull skips is missed by every ray of the light's sampling cone (rim u = 1 and axis
    included), per the oracle; root_occluded_fast with those skip bits still equals the oracle's occlusion test --
    shading points on surfaces and in the free space of the scene"""
    sc, flat, roles, handles = qscene
    rs, a = scene_sets
    rng = np.random.default_rng(17)
    fin = np.isfinite(a)
    pts = np.concatenate([R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], a[fin])[:400], rng.uniform(-4, 4, (200, 3))])
    counts = cone_check(handles["default"], flat, oracle, pts, [None] * len(pts), rng)
    print("cone culls, random points:", dict(counts))
    assert counts["culled"] > 100


def test_cone_cull_at_tangency(qscene, oracle):
    """the margins of root_cone_cull: shading points from which an element's sphere or envelope touches the light's cone
    from outside (internal common tangents of the two balls, built in mpmath: cos_phi = cos_sum), points on an element's
    ball and one and a few ulps off it (L2 = R2), and points from which a rim generator is parallel to a plane element
    (d_min or d_max = 0).  The rays include the rim generator along the tangent line, in the device's own frame."""
    sc, flat, roles, handles = qscene
    rng = np.random.default_rng(19)
    light = flat.elems_of(flat.c.light_root)[0]
    lpos, lr = np.array(flat.node(light).pos[:]), float(flat.node(light).prm[0])
    pts, lines = [], []
    for e in flat.elems_of(flat.c.matter_root)[:64]:
        n = flat.node(e)
        if (n.flags & 1) or n.type == R.ACN_SPHERE:
            c, rad = R.node_ball(flat, e)
            for p, d in R.cone_tangent_balls(rng, lpos, lr, c, rad):
                pts.append(p); lines.append(d)
            for k in (-2, 0, 1, 2, 4, 64):   # on the ball, seen towards the light
                u = R.unit(R.unit(lpos - c) + 0.6 * R.random_dirs(rng, 3))
                for uu in u:
                    pts.append(c + uu * (rad * (1 + k * R.ULP))); lines.append(None)
        elif n.type == R.ACN_PLANE:
            for p, d in R.cone_parallel_plane(rng, lpos, lr, R.rax(n)[2]):
                pts.append(p); lines.append(d)
    counts = cone_check(handles["default"], flat, oracle, np.array(pts), lines, rng, n_random=4)
    print("cone culls at tangency:", dict(counts))
    assert counts["points"] > 150 and counts["rim_hits"] > 20


# ---- 7. simple compounds ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{}, {"ACN_NO_SC_CULL": 1}, {"ACN_NO_SC_REVERSED": 1}], ids=["culled", "no_cull", "one_order"])
def test_simple_compounds(env, oracle):
    """simple_compound_hit (culled walk with the reversed table, no culling, the single-order table) returns the
    oracle's compound_s_ray_hit distance, normal and hit object -- on the tie compound (every sphere twice, distances
    tie bit for bit) and on many_spheres tables"""
    rng = np.random.default_rng(23)
    sc, roles = R.query_scene(seed=1)
    scenes = [("ties", sc)]
    for name in ("many_spheres:3:0", "many_spheres:4:1"):
        scenes.append((name, A.Scene.build(name)))
    ties_total = 0
    for name, s in scenes:
        flat = s.flatten()
        h = upload(flat, **env)
        info = h.query_rays("elements", flat.c.matter_root, n=len(flat.elems_of(flat.c.matter_root)))
        scs = [int(info[k, 0]) for k in range(len(info)) if int(info[k, 1]) & 4]
        assert scs, name
        for e in scs:
            c, rad = R.node_ball(flat, e, default_r=3.0)
            rs = R.uniform(rng, c, rad, 3000)
            a, nor, ho = oracle.compound_ray_hits(flat, e, rs.rays)
            rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=100))
            leaves = R.leaves_of(flat, e)
            cen = np.array([flat.node(l).pos[:] for l in leaves[:200]])
            d = R.random_dirs(rng, len(cen))
            rs.add(np.concatenate([cen - 4 * d, d], axis=1), "ties")   # through leaf centres: duplicates tie exactly
            rs.add(np.concatenate([cen + 4 * d, -d], axis=1), "ties")
            z = np.tile([0.0, 0.0, 1.0], (len(cen), 1))   # along the shift of the near twins, both ways, slightly off centre
            for off in (0.0, 0.05, 0.1):
                o = cen + off * R.random_dirs(rng, len(cen))
                rs.add(np.concatenate([o - 4 * z, z], axis=1), "ties")
                rs.add(np.concatenate([o + 4 * z, -z], axis=1), "ties")
            a, nor, ho = oracle.compound_ray_hits(flat, e, rs.rays)
            fin = np.isfinite(a)
            for lds in (True, False):
                g = h.query_rays("sc_hit", e, rs.rays, limits=np.where(fin, a, 1.0), lds=lds)
                bad = (bits(g[:, 0]) != bits(a)) | (fin & ((g[:, 4] != ho) | (bits(g[:, 1:4]) != bits(nor)).any(axis=1)))
                assert not bad.any(), report_mismatch(f"simple_compound_hit {env} lds={lds}", f"{name} element {e}", rs, bad)
                anyhit = g[:, 5] != 0
                assert (anyhit == fin).all(), f"simple_compound_hit any-hit form {env} on {name}"
            if name == "ties":
                pos = {l: tuple(flat.node(l).pos[:]) + (flat.node(l).prm[0],) for l in leaves}
                twins = Counter(pos.values())
                ties_total += int(sum(twins[pos[int(k)]] > 1 for k in ho[fin & (rs.cls == "ties")]))
        h.close()
    print(f"simple compounds {env}: hits on a leaf that has an identical twin: {ties_total}")
    assert ties_total > 50


# ---- 8. wave independence -----------------------------------------------------------------------------------------

def test_wave_independence(qscene, element_sets):
    """the same rays as generated, grouped by outcome and shuffled: every ray gets the same answer in every order (which
    rays share a wave must not change any result of the lock-step machines or the wave-uniform pre-tests)"""
    sc, flat, roles, handles = qscene
    h = handles["prune_min_1"]
    rng = np.random.default_rng(31)
    for (role, e), (rs, a, nor) in element_sets.items():
        if flat.node(e).type not in MACHINE_TYPES:
            continue
        orders = [np.arange(len(rs)), np.argsort(np.isfinite(a), kind="stable"), rng.permutation(len(rs))]
        for op in ("hit_uni", "side_uni", "prune", "element_hit"):
            ref = None
            for order in orders:
                g = h.query_rays(op, e, rs.rays[order])
                res = np.empty_like(g)
                res[order] = g
                if ref is None:
                    ref = res
                else:
                    bad = (bits(res) != bits(ref)).any(axis=1)
                    assert not bad.any(), report_mismatch(f"{op} depends on the order of the rays", role, rs, bad)


# ---- both node placements ----------------------------------------------------------------------------------------

def test_lds_staged_nodes(oracle):
    """The handles above read their nodes from global memory (the upload step stages nodes in LDS only for small scenes
    whose roots hold generic nested compounds).  A scene that is staged: the hit, side and root queries with the nodes in
    LDS and in global memory, against the oracle."""
    import ctypes as C
    from actinon_amd._lib import host
    rng = np.random.default_rng(41)
    sc = A.Scene()
    sc.set(image_width=32, image_height=24, direct_samples=4, path_samples=2)
    light = host.acn_obj_sphere_s_create(0.5)
    host.acn_obj_set_radiance(light, 20.0)
    host.acn_obj_move(light, A.v3(0, -2, 5))
    sc.push(light); host.acn_obj_discard(light)
    a = R.make_leaf("ellipsoid", rng)
    b = R.make_leaf("cylinder", rng)
    pair = host.acn_obj_pair_inside_s_create_pair(a, b)
    cmp = host.acn_compound_s_create()
    host.acn_compound_s_push(cmp, pair)
    s2 = host.acn_obj_sphere_s_create(0.4)
    host.acn_obj_move(s2, A.v3(0.8, 0, 0.3))
    host.acn_compound_s_push(cmp, s2)
    host.acn_obj_set_envelope(cmp, A.v3(0, 0, 0), 2.5)
    sc.push(cmp)
    smp = host.acn_compound_s_create()   # a simple compound: simple_compound_hit reads its nodes from LDS too
    for k in range(2):
        t = host.acn_obj_sphere_s_create(0.3)
        host.acn_obj_move(t, A.v3(-0.4 + 0.5 * k, 1.0, -0.2))
        host.acn_obj_set_envelope(t, A.v3(-0.4 + 0.5 * k, 1.0, -0.2), 0.3 * (1 + 4e-9))
        host.acn_compound_s_push(smp, t)
        host.acn_obj_discard(t)
    host.acn_obj_set_envelope(smp, A.v3(0, 1.0, -0.2), 1.0)
    sc.push(smp)
    for o in (a, b, pair, s2, cmp, smp):
        host.acn_obj_discard(o)
    flat = sc.flatten()
    h = upload(flat, ACN_PRUNE_MIN=1)   # the CSG pair gets an interval-prune program
    root = flat.c.matter_root
    info = h.query_rays("elements", root, n=2)
    assert info[0, 3] > 0, "the scene was not staged in LDS"
    comp, simple = flat.elems_of(root)[:2]
    csg = flat.elems_of(comp)[0]
    assert int(info[1, 1]) & 4   # the second element is a simple compound
    skipped, sc_hits = {}, {}
    rs = R.uniform(rng, np.zeros(3), 2.0, 4000)
    a, nor = oracle.obj_ray_hits(flat, csg, rs.rays)
    rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=100))
    for leaf in R.leaves_of(flat, csg):
        if flat.node(leaf).type == R.ACN_SQUAROID:
            rs.extend(R.degenerate(rng, flat.node(leaf), 50))
            rs.add(R.squaroid_tangent_lines(flat.node(leaf), rng, 30, digits=30)[0], "tangent")
    a, nor = oracle.obj_ray_hits(flat, csg, rs.rays)
    ta, tn, tex, ten = oracle.trans_hits(flat, root, rs.rays)
    ca, _, _ = oracle.compound_ray_hits(flat, root, rs.rays)
    sides = oracle.obj_sides(flat, csg, rs.rays[:, :3])
    fin = np.isfinite(a)
    for lds in (True, False):
        for op in ("hit_lane", "hit_uni", "element_hit"):
            g = h.query_rays(op, csg, rs.rays, lds=lds)
            bad = (bits(g[:, 0]) != bits(a)) | (fin & (bits(g[:, 1:4]) != bits(nor)).any(axis=1))
            assert not bad.any(), report_mismatch(f"{op} lds={lds} (staged scene)", "csg", rs, bad)
        for op in ("side_lane", "side_uni"):
            assert (h.query_rays(op, csg, rs.rays, lds=lds)[:, 0] == sides).all(), (op, lds)
        g = h.query_rays("trans", root, rs.rays, lds=lds)
        for off in (0, 6):
            assert (bits(g[:, off]) == bits(ta)).all() and ((g[:, off + 4] == tex) | ~np.isfinite(ta)).all(), (off, lds)
        lim = np.where(np.isfinite(ca), ca, 1.0)
        o = h.query_rays("occluded", root, rs.rays, limits=lim, lds=lds)
        assert ((o[:, 0] != 0) == (ca <= lim)).all(), lds
        pr = h.query_rays("prune", csg, rs.rays, limits=np.full(len(rs), np.inf), lds=lds)
        assert (pr[:, 3] == 1).all()   # the program exists
        assert not (((pr[:, 0] != 0) | (pr[:, 2] != 0)) & fin).any(), lds
        skipped[lds] = int((pr[:, 2] != 0).sum())
        sa, sn, sho = oracle.compound_ray_hits(flat, simple, rs.rays)
        g = h.query_rays("sc_hit", simple, rs.rays, lds=lds)
        sf = np.isfinite(sa)
        assert (bits(g[:, 0]) == bits(sa)).all() and (g[sf, 4] == sho[sf]).all(), lds
        sc_hits[lds] = int(sf.sum())
    assert skipped[True] == skipped[False] > 100 and sc_hits[True] > 100, (skipped, sc_hits)
    h.close()

"""CPU checks of the per-query test machinery (tests/test_gpu_queries.py): the oracle's batch entry equals its one-ray
functions, and the ray generators of tests/ray_sets.py produce what they claim."""
from collections import Counter

import mpmath as mp
import numpy as np
import pytest

import ray_sets as R


@pytest.fixture(scope="module")
def qscene():
    sc, roles = R.query_scene(seed=1)
    return sc, sc.flatten(), roles


def sample_sets(oracle, flat, rng):
    """a few rays of every class on a sphere, a squaroid, a plane and a CSG element"""
    els = flat.elems_of(flat.c.matter_root)
    out = []
    for e in (els[0], els[6], els[7], els[10]):
        c, rad = R.node_ball(flat, e)
        rs = R.uniform(rng, c, rad, 200)
        a, nor = oracle.obj_ray_hits(flat, e, rs.rays)
        rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=20))
        rs.extend(R.tangent_ball(rng, c, rad, 5))
        rs.extend(R.far(rng, c, rad, 20))
        rs.extend(R.envelope_boundary(rng, c, rad, 5))
        for leaf in R.leaves_of(flat, e)[:3]:
            ln = flat.node(leaf)
            if ln.type == R.ACN_SQUAROID:
                rs.add(R.squaroid_tangent_lines(ln, rng, 4, digits=30)[0], "tangent")
                rs.extend(R.degenerate(rng, ln, 5))
            elif ln.type == R.ACN_PLANE:
                rs.extend(R.plane_parallel(rng, ln, 5))
        out.append((e, rs))
    return out


def test_oracle_batch_equals_one_ray_functions(oracle, qscene):
    sc, flat, roles = qscene
    rng = np.random.default_rng(2)
    sets = sample_sets(oracle, flat, rng)
    classes = set()
    for e, rs in sets:
        a, nor = oracle.obj_ray_hits(flat, e, rs.rays, threads=4)
        sides = oracle.obj_sides(flat, e, rs.rays[:, :3], threads=4)
        for k in range(len(rs)):
            a1, n1 = oracle.obj_ray_hit(flat, e, rs.rays[k, :3], rs.rays[k, 3:])
            assert np.float64(a1).view(np.uint64) == a[k].view(np.uint64), (e, rs.cls[k])
            assert (np.asarray(n1).view(np.uint64) == nor[k].view(np.uint64)).all()
            assert oracle.obj_side(flat, e, rs.rays[k, :3]) == sides[k]
        classes |= set(rs.cls)
    assert {"uniform", "secondary", "secondary_walk", "tangent", "degenerate", "far", "envelope"} <= classes
    # trans_hit of the matter root: the one-ray export runs the light root first, so compare on rays the light root misses
    root = flat.c.matter_root
    rays = np.concatenate([rs.rays for _, rs in sets])
    ta, tn, tex, ten = oracle.trans_hits(flat, root, rays)
    la, _ = oracle.obj_ray_hits(flat, flat.elems_of(flat.c.light_root)[0], rays)
    ca, cn, cho = oracle.compound_ray_hits(flat, root, rays)
    occ = oracle.query_rays(flat, "occluded", root, rays, limits=ca)[:, 5]
    assert (occ[np.isfinite(ca)] == 1).all()
    for k in np.flatnonzero(~np.isfinite(la))[:400]:
        a1, n1, ex, en = oracle.trans_hit(flat, rays[k, :3], rays[k, 3:])
        assert np.float64(a1).view(np.uint64) == ta[k].view(np.uint64)
        if np.isfinite(a1):
            assert (ex, en) == (tex[k], ten[k]) and (np.asarray(n1).view(np.uint64) == tn[k].view(np.uint64)).all()
            assert cho[k] in (ex, en)   # the nearest hit object is the one entered or left


def test_tangent_balls_within_stated_ulps():
    """lines of the tangent class lie at R ( 1 + k 2^-52 ) from the centre, to a few ulps of R (rounding of the foot point)"""
    rng = np.random.default_rng(4)
    c, rad = np.array([0.3, -1.2, 2.5]), 0.75
    rs = R.tangent_ball(rng, c, rad, 10)
    mp.mp.dps = 50
    ks = [k for k in R.TANGENT_K for _ in range(20)]
    for (ray, k) in zip(rs.rays, ks):
        p = [mp.mpf(float(v)) for v in ray[:3]]
        d = [mp.mpf(float(v)) for v in ray[3:]]
        dd = mp.fsum(x * x for x in d)
        w = [p[i] - mp.mpf(float(c[i])) for i in range(3)]
        s = mp.fsum(w[i] * d[i] for i in range(3)) / dd
        dist = mp.sqrt(mp.fsum((w[i] - s * d[i]) ** 2 for i in range(3)))
        ulps = float((dist / rad - 1) / mp.mpf(2) ** -52)
        assert abs(ulps - k) <= 8 + 1e-6 * abs(k), (k, ulps)


def test_squaroid_tangent_lines_touch_the_surface(qscene):
    """the quadric restricted to a tangent line has a (near) double root: its discriminant is tiny against B^2"""
    sc, flat, roles = qscene
    rng = np.random.default_rng(6)
    mp.mp.dps = 50
    done = Counter()
    for e in flat.elems_of(flat.c.matter_root)[1:7]:   # ellipsoid, hyperboloids, cone, cylinder, general squaroid
        n = flat.node(e)
        rays, pts = R.squaroid_tangent_lines(n, rng, 6)
        M = mp.matrix(R.rax(n).tolist())
        pos = mp.matrix([float(v) for v in n.pos[:]])
        a, b, c, r = (mp.mpf(float(v)) for v in n.prm[:4])
        for ray in rays:
            p = M * (mp.matrix([mp.mpf(float(v)) for v in ray[:3]]) - pos)
            d = M * mp.matrix([mp.mpf(float(v)) for v in ray[3:]])
            A = a * d[0] ** 2 + b * d[1] ** 2 + c * d[2] ** 2
            B = a * p[0] * d[0] + b * p[1] * d[1] + c * p[2] * d[2]
            Cc = a * p[0] ** 2 + b * p[1] ** 2 + c * p[2] ** 2 + r
            disc = B * B - A * Cc
            scale = B * B + abs(A * Cc) + mp.mpf(1e-30)
            assert abs(disc) / scale < 1e-13, (e, float(disc / scale))
            done[e] += 1
    assert len(done) == 6 and min(done.values()) >= 3


def test_secondary_origins_are_ray_pos_and_ties_are_exact(oracle, qscene):
    sc, flat, roles = qscene
    rng = np.random.default_rng(8)
    e = flat.elems_of(flat.c.matter_root)[0]
    c, rad = R.node_ball(flat, e)
    rs = R.uniform(rng, c, rad, 300)
    a, nor = oracle.obj_ray_hits(flat, e, rs.rays)
    sec = R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=10)
    fin = np.isfinite(a)
    rp, rd, af = rs.rays[fin, :3], rs.rays[fin, 3:], a[fin]
    want = np.empty_like(rp)
    for k in range(len(af)):   # ray_pos (vectors.h:343-346) one component at a time
        want[k] = [rp[k, i] + rd[k, i] * af[k] for i in range(3)]
    got = sec.rays[sec.cls == "secondary"][:len(af), :3]
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    walk = sec.rays[sec.cls == "secondary_walk"][:len(af), :3]
    want2 = np.array([[rp[k, i] + rd[k, i] * (af[k] + 2 * R.F3_EPS) for i in range(3)] for k in range(len(af))])
    assert (walk.view(np.uint64) == want2.view(np.uint64)).all()
    # the tie compound holds every sphere twice, bit for bit, under different parents
    ties = flat.elems_of(flat.c.matter_root)[roles.index("ties")]
    leaves = R.leaves_of(flat, ties)
    key = Counter(np.array(list(flat.node(l).pos[:]) + [flat.node(l).prm[0]]).tobytes() for l in leaves)
    assert len(leaves) == 64 and set(key.values()) == {2}
    # and a ray through a sphere's centre gets the same distance from both copies
    l0 = leaves[0]
    twin = [l for l in leaves if l != l0 and flat.node(l).pos[:] == flat.node(l0).pos[:]][0]
    ray = np.concatenate([np.array(flat.node(l0).pos[:]) - [0, 0, 3], [0, 0, 1.0]])
    a0, _ = oracle.obj_ray_hit(flat, l0, ray[:3], ray[3:])
    a1, _ = oracle.obj_ray_hit(flat, twin, ray[:3], ray[3:])
    assert np.isfinite(a0) and np.float64(a0).view(np.uint64) == np.float64(a1).view(np.uint64)


def test_plane_parallel_rays_are_exact(qscene):
    """nor . rd, as the device evaluates it, is exactly 0 for the untilted rays and has the sign of every tilt"""
    sc, flat, roles = qscene
    n = flat.node(flat.elems_of(flat.c.matter_root)[roles.index("plane")])
    nor = R.rax(n)[2]
    m = 30
    rs = R.plane_parallel(np.random.default_rng(3), n, m)
    assert len(rs) == m * 3 * len(R.PLANE_TILTS)
    dots = np.array([R.dot_dev(nor, d) for d in rs.rays[:, 3:]])
    for k, tilt in enumerate(R.PLANE_TILTS):
        v = dots[k * 3 * m:(k + 1) * 3 * m]
        if tilt == 0:
            assert (v == 0).all()
        else:
            assert (np.sign(v) == np.sign(tilt)).all(), (tilt, v)
            if abs(tilt) == 1:
                assert np.abs(v).max() < 1e-15   # the smallest tilt: a rounding step of the dot product
        assert (np.abs(np.linalg.norm(rs.rays[k * 3 * m:(k + 1) * 3 * m, 3:], axis=1) - 1) < 1e-12).all()


def test_cone_tangent_points_touch_both_balls():
    """the shading points of the tangency class lie on a line tangent to the light and to the element's ball, with the
    ball on the other side of the line (it touches the light's cone from outside)"""
    rng = np.random.default_rng(5)
    lc, lr, c, r = np.array([-1.0, -2.0, 7.0]), 0.7, np.array([0.5, 0.3, 1.0]), 0.9
    cfg = R.cone_tangent_balls(rng, lc, lr, c, r)
    assert len(cfg) == 18
    mp.mp.dps = 40
    for p, d in cfg:
        P = [mp.mpf(float(v)) for v in p]
        Dd = [mp.mpf(float(v)) for v in d]
        for cc, rr in ((lc, lr), (c, r)):
            w = [mp.mpf(float(cc[i])) - P[i] for i in range(3)]
            s = mp.fsum(w[i] * Dd[i] for i in range(3))
            assert s > 0   # both tangent points lie ahead
            dist = mp.sqrt(mp.fsum((w[i] - s * Dd[i]) ** 2 for i in range(3)))
            assert abs(dist / rr - 1) < 1e-14
        # opposite sides: the two centres' offsets from the line point away from each other
        off = []
        for cc in (lc, c):
            w = np.array(cc) - p
            off.append(w - np.dot(w, d) * d)
        assert np.dot(off[0], off[1]) < 0

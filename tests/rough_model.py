"""The two references of the rough-surface and distance-object tests, independent of the oracle's and the device's code:

  exact_torus_sdf / exact_torus_normal   the torus of a distance node in closed form, in longdouble
  roughen                                the perturbation of a rough surface's normal (objects.c:266-282), in numpy

and check_rough_steps, which applies roughen node by node to whatever computes hits (the oracle or a device handle)."""
import numpy as np

import ray_sets as R

OP_LOG, OP_SQRT = 4, 7        # op codes of tests/csrc/detmath_cpu.c
# bcore_lcg00_u3, as include/actinon_hip.h declares it (ACN_LCG00_A, ACN_LCG00_C)
LCG00_A, LCG00_C = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
SEED = 1246


def _local(node, points):
    L = np.longdouble
    p = np.asarray(points, dtype=L).reshape(-1, 3) - np.array(node.pos[:], dtype=L)
    return (p @ R.rax(node).astype(L).T) * L(node.prm[0])


def exact_torus_sdf(node, points):
    """the signed distance of world points to the torus of distance node `node`, in world units (longdouble): local
    coordinates rax ( p - pos ) inv_scale, radii 1 and prm[1] there, the local distance divided by inv_scale = prm[0]"""
    q = _local(node, points)
    rho = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - 1
    return (np.sqrt(rho ** 2 + q[:, 2] ** 2) - np.longdouble(node.prm[1])) / np.longdouble(node.prm[0])


def exact_torus_normal(node, points):
    """the unit gradient of exact_torus_sdf at world points (longdouble)"""
    q = _local(node, points)
    f = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2)
    g = np.stack([q[:, 0] * (1 - 1 / f), q[:, 1] * (1 - 1 / f), q[:, 2]], axis=1)
    g = g / np.sqrt((g ** 2).sum(axis=1))[:, None]
    return g @ R.rax(node).astype(np.longdouble)


def on_torus_axis(node, points):
    """True where a world point lies on the torus' axis (local x = y = 0, to 1e-12).  There the reference's torus function
    (distance.c:83-92: f = sqrt( x^2 + y^2 ), f_inv = f > 0 ? 1 / f : 1) is NOT the torus: with f == 0 it returns | z | - prm[1], a
    ball of the tube's radius about the centre that exists on the axis alone.  The oracle and the device follow it; the exact
    references leave such points out, and test_axis_function pins what the reference does there."""
    q = _local(node, points)
    return np.asarray(np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) < 1e-12)


def det(lib, op, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.detmath_eval(op, x.ctypes.data, None, out.ctypes.data, x.size)
    return out


def of_length_1(lib, v):
    """v_of_length( v, 1.0 ) (vectors.h:148-154): unchanged where | |v|^2 - 1 | < 1e-8, else v * ( 1 / sqrt( |v|^2 ) )"""
    r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    with np.errstate(all="ignore"):
        f = np.where(r2 > 0, 1.0 / det(lib, OP_SQRT, r2), 0.0)
    return np.where((np.abs(r2 - 1.0) < 1e-8)[:, None], v, v * f[:, None])


def roughen(normal, hit_pos, roughness, oracle, detmath_cpu):
    """objects.c:266-282: rv = v_random_seed( hit_pos, 1246 ); per component f = f3_rnd0( &rv ) * 0.99,
    n += roughness * log( ( 1 - f ) / ( 1 + f ) ); then v_of_length( n, 1 ).  f3_rnd0 steps rv = rv * A + C in uint64 and
    returns (double) rv * ( 2 / 2^64 ) - 1; log and sqrt are those of acn_detmath.h, built for the host."""
    n = np.array(normal, dtype=np.float64).reshape(-1, 3)
    pos = np.ascontiguousarray(hit_pos, dtype=np.float64).reshape(-1, 3)
    rv = np.array([oracle.random_seed(p, SEED) for p in pos], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(3):
            rv = rv * LCG00_A + LCG00_C
            f = (rv.astype(np.float64) * (2.0 / float(0xFFFFFFFFFFFFFFFF)) - 1.0) * 0.99
            n[:, k] = n[:, k] + roughness * det(detmath_cpu, OP_LOG, (1.0 - f) / (1.0 + f))
    return of_length_1(detmath_cpu, n)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _mlv(M, v):
    """m_mlv: row . v, summed left to right"""
    return np.stack([(M[k, 0] * v[:, 0] + M[k, 1] * v[:, 1]) + M[k, 2] * v[:, 2] for k in range(3)], axis=1)


def _tmlv(M, v):
    return np.stack([(M[0, k] * v[:, 0] + M[1, k] * v[:, 1]) + M[2, k] * v[:, 2] for k in range(3)], axis=1)


def scale_rays(lib, node, rays):
    """the ray a scale wrapper hands to its operand (objects.c:1418-1437): origin and direction in the wrapper's frame times
    inv_scale, the direction brought to length 1 by d * ( 1 / sqrt( d . d ) )"""
    M, inv = R.rax(node), np.array(node.prm[:3])
    p = _mlv(M, rays[:, :3] - np.array(node.pos[:])) * inv
    d = _mlv(M, rays[:, 3:]) * inv
    ln = det(lib, OP_SQRT, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        f = np.where(ln > 0, 1.0 / ln, 0.0)
    return np.concatenate([p, d * f[:, None]], axis=1)


def check_rough_steps(flat, twin, node, rays, hits, twin_hits, sides, oracle, lib, stats, path=""):
    """The model of a rough normal, one node at a time.  hits( node, rays ) -> ( a, nor ) evaluates a node of the rough scene,
    twin_hits the same node of the smooth twin, sides( node, points ) is obj_side.  For every node of the subtree of `node`, on
    the rays that reach it:
      a leaf              nor == roughen( twin's nor )                       at ray_pos( rp, rd, a )
      NEG( c )            nor == roughen( -nor_c )                           at ray_pos( rp, rd, a )
      a pair ( c0, c1 )   nor == roughen( nor of the operand whose hit it is )  at ray_pos( rp, rd, a ), for the hits that
                          are an operand's hit of the pair's own ray (objects.c:1057-1073: a0 < a1 and c1's side at a0 is the
                          wanted one, else c0's side at a1 is).  The hits of the alternating walk (objects.c:1075-1092) start
                          from a moved origin, whose operand hit seeds with a position of other bits: they are counted in
                          stats["walk"] and left to the oracle comparison
      SCALE( c )          the operand sees scale_rays(): ITS roughness is seeded by the hit position in the scaled frame,
                          ray_pos( p', d', a_c ); the wrapper's normal is v_of_length( rax^T ( nor_c * inv_scale ) ) and its own
                          roughness is seeded in the outer frame
    each with the node's own roughness where that is > 0 -- operand first, parent last, by induction over the tree.
    Returns the number of normals that differ from the model; stats counts the rays checked per kind of step."""
    n = flat.node(node)
    if not len(rays):
        return 0
    a, nor = hits(node, rays)
    fin = np.isfinite(a)
    bad = 0
    t = n.type
    if t in (R.ACN_PLANE, R.ACN_SPHERE, R.ACN_SQUAROID, R.ACN_DISTANCE):
        ta, base = twin_hits(node, rays)
        bad += int((bits(ta) != bits(a)).sum())
        use = fin
        kind = "leaf"
    elif t == R.ACN_NEG:
        ca, cn = hits(n.child0, rays)
        base, use, kind = -cn, fin & (bits(ca) == bits(a)), "neg"
        bad += check_rough_steps(flat, twin, n.child0, rays, hits, twin_hits, sides, oracle, lib, stats, path + "!")
    elif t in (R.ACN_PAIR_INSIDE, R.ACN_PAIR_OUTSIDE):
        a0, n0 = hits(n.child0, rays)
        a1, n1 = hits(n.child1, rays)
        want_side = -1 if t == R.ACN_PAIR_INSIDE else 1
        first = fin & (a0 < a1)   # (not finite: the pair's own envelope turned the ray away)
        first[first] = sides(n.child1, R.ray_pos(rays[first, :3], rays[first, 3:], a0[first])) == want_side
        second = fin & ~first & np.isfinite(a1)
        second[second] = sides(n.child0, R.ray_pos(rays[second, :3], rays[second, 3:], a1[second])) == want_side
        base = np.where(first[:, None], n0, n1)
        use, kind = first | second, "pair"
        bad += int((bits(np.where(first, a0, a1))[use] != bits(a)[use]).sum())
        stats["walk"] = stats.get("walk", 0) + int((fin & ~use).sum())
        bad += check_rough_steps(flat, twin, n.child0, rays, hits, twin_hits, sides, oracle, lib, stats, path + "0")
        bad += check_rough_steps(flat, twin, n.child1, rays, hits, twin_hits, sides, oracle, lib, stats, path + "1")
    elif t == R.ACN_SCALE:
        inner = scale_rays(lib, n, rays)
        ca, cn = hits(n.child0, inner)
        base = of_length_1(lib, _tmlv(R.rax(n), cn * np.array(n.prm[:3])))
        use, kind = fin & np.isfinite(ca), "scale"
        bad += check_rough_steps(flat, twin, n.child0, inner, hits, twin_hits, sides, oracle, lib, stats, path + "*")
    else:
        raise AssertionError(f"no model for node type {t}")
    if use.any():
        want = base[use]
        if n.surface_roughness > 0:
            want = roughen(want, R.ray_pos(rays[use, :3], rays[use, 3:], a[use]), float(n.surface_roughness), oracle, lib)
            stats["rough_" + kind] = stats.get("rough_" + kind, 0) + int(use.sum())
        else:
            stats["smooth_" + kind] = stats.get("smooth_" + kind, 0) + int(use.sum())
        d = (bits(want) != bits(nor[use])).any(axis=1)
        if d.any():
            stats.setdefault("first_bad", (path, node, int(t), rays[use][np.flatnonzero(d)[0]].tolist()))
        bad += int(d.sum())
    return bad

"""Seeded objects and ray sets aimed at the margins of the device's traversal shortcuts (tests/test_gpu_queries.py).

Every generator returns a RaySet: rays [n, 6] (origin, unit direction) and a class label per ray, so that failures and
coverage are reported per class:
  uniform     origins in 1.5x the element's bounding ball, random directions                        (a)
  secondary   origins at ray_pos( rp, rd, a ) of oracle hits and a + 2 f3_eps beyond, directions:
              reflection, refraction (the oracle's fresnel_refraction), both hemispheres            (b)
  tangent     lines at distance R (1 + k 2^-52) from ball centres; tangent lines of quadrics built in
              mpmath at 50 digits; rays parallel to planes (nor . rd = 0 and +-tiny)                 (c)
  degenerate  rays through cone apices and along the axes of cylinders and hyperboloids             (d)
  far         origins 1e3 .. 1e6 away, aimed at the element                                         (e)
  envelope    origins on an envelope sphere and +-1 ulp off it                                      (f)
  rim         directions of a light's sampling cone, rim and axis included                          (i)
Limits for occlusion (g) come from occlusion_limits(); the exact ties (h) from tie_compound()."""
import ctypes as C

import numpy as np

import actinon_amd as A
from actinon_amd._lib import host

F3_EPS = 1e-6
ULP = 2.0 ** -52
TANGENT_K = (-64, -1, 0, 1, 64, 2 ** 20)

ACN_PLANE, ACN_SPHERE, ACN_SQUAROID, ACN_DISTANCE, ACN_PAIR_INSIDE, ACN_PAIR_OUTSIDE, ACN_NEG, ACN_SCALE, ACN_COMPOUND = range(1, 10)


class RaySet:
    def __init__(self, rays=None, cls=None):
        self.rays = np.zeros((0, 6)) if rays is None else np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        self.cls = np.array([], dtype=object) if cls is None else np.asarray(cls, dtype=object)

    def __len__(self):
        return self.rays.shape[0]

    def add(self, rays, label):
        rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
        ok = np.isfinite(rays).all(axis=1) & (np.abs(np.linalg.norm(rays[:, 3:], axis=1) - 1) < 1e-12)
        rays = rays[ok]
        self.rays = np.concatenate([self.rays, rays])
        self.cls = np.concatenate([self.cls, np.array([label] * len(rays), dtype=object)])
        return self

    def extend(self, other):
        self.rays = np.concatenate([self.rays, other.rays])
        self.cls = np.concatenate([self.cls, other.cls])
        return self

    def classes(self):
        return sorted(set(self.cls))


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_dirs(rng, n):
    return unit(rng.normal(size=(n, 3)))


def ray_pos(p, d, a):
    """vectors.h:343-346 in the renderer's order: p + d * a, component by component (no contraction)."""
    return p + d * np.asarray(a)[..., None]


def reflection(d, nor):
    """v_reflection (vectors.h:238-241)."""
    return unit(d - nor * (2.0 * np.sum(d * nor, axis=-1, keepdims=True)))


# ---------------------------------------------------------------------------------------------------------------------
# objects

def _rot(rng):
    m = host.acn_rotx(float(rng.uniform(0, 360)))
    m2 = host.acn_roty(float(rng.uniform(0, 360)))
    m3 = host.acn_rotz(float(rng.uniform(0, 360)))
    return (m, m2, m3)


def _place(o, rng, spread=0.6, rotate=True):
    if rotate:
        for m in _rot(rng):
            host.acn_obj_rotate(o, C.byref(m))
    host.acn_obj_move(o, A.v3(*rng.uniform(-spread, spread, 3)))
    return o


LEAF_KINDS = ("sphere", "ellipsoid", "hyperboloid1", "hyperboloid2", "cone", "cylinder", "squaroid", "plane")


def make_leaf(kind, rng):
    s = lambda lo=0.3, hi=1.0: float(rng.uniform(lo, hi))  # noqa: E731
    if kind == "sphere":
        o = host.acn_obj_sphere_s_create(s())
    elif kind == "ellipsoid":
        o = host.acn_obj_squaroid_s_create_ellipsoid(s(), s(), s())
    elif kind == "hyperboloid1":
        o = host.acn_obj_squaroid_s_create_hyperboloid1(s(), s(), s())
    elif kind == "hyperboloid2":
        o = host.acn_obj_squaroid_s_create_hyperboloid2(s(), s(), s())
    elif kind == "cone":
        o = host.acn_obj_squaroid_s_create_cone(s(), s(), s())
    elif kind == "cylinder":
        o = host.acn_obj_squaroid_s_create_cylinder(s(), s())
    elif kind == "squaroid":
        o = host.acn_obj_squaroid_s_create_squaroid(s(0.5, 2), -s(0.5, 2), s(0.5, 2), -s(0.1, 0.5))
    elif kind == "plane":
        o = host.acn_obj_plane_s_create()
    else:
        raise ValueError(kind)
    host.acn_obj_set_material(o, b"diffuse")
    return _place(o, rng)


def random_csg(rng, depth, leaf=None, visit=None):
    """A random CSG tree of the given depth over every primitive constructor, with complements, scale wrappers,
    rotations, moves and explicit envelopes on the way.  leaf( kind, rng ) replaces make_leaf; visit( o ) sees every leaf
    and every pair before its parent clones it (neither may draw from rng: the tree stays the same)."""
    leaf = leaf or make_leaf
    visit = visit or (lambda o: None)
    if depth == 0:
        o = leaf(LEAF_KINDS[int(rng.integers(0, len(LEAF_KINDS)))], rng)
        visit(o)
        return o
    a = random_csg(rng, depth - 1, leaf, visit)
    b = random_csg(rng, int(rng.integers(0, depth)), leaf, visit)
    # a bounded operand keeps the infinite quadrics and half-spaces from filling the scene
    if rng.random() < 0.5:
        ball = host.acn_obj_sphere_s_create(float(rng.uniform(0.8, 1.4)))
        host.acn_obj_move(ball, A.v3(*rng.uniform(-0.3, 0.3, 3)))
        t = host.acn_obj_pair_inside_s_create_pair(b, ball)
        host.acn_obj_discard(b); host.acn_obj_discard(ball)
        b = t
    if rng.random() < 0.2:
        t = host.acn_obj_neg_s_create_neg(b)
        host.acn_obj_discard(b)
        b = t
    inside = rng.random() < 0.6
    o = (host.acn_obj_pair_inside_s_create_pair if inside else host.acn_obj_pair_outside_s_create_pair)(a, b)
    host.acn_obj_discard(a); host.acn_obj_discard(b)
    visit(o)
    if rng.random() < 0.15:
        t = host.acn_obj_scale_s_create_scale(o, A.v3(*rng.uniform(0.6, 1.5, 3)))
        host.acn_obj_discard(o)
        o = t
    if rng.random() < 0.3:
        # explicit envelopes: generous ones and ones that clip the object (both are legal in the reference)
        host.acn_obj_set_envelope(o, A.v3(*rng.uniform(-0.3, 0.3, 3)), float(rng.uniform(0.9, 2.5)))
    return o


def plane_normal(p):
    """the normal of plane object p as the flattened scene holds it (rax row z)"""
    sc = A.Scene()
    sc.push(p)
    f = sc.flatten()
    return rax(f.node(f.elems_of(f.c.matter_root)[0]))[2].copy()


def balanced_polytope(rng, n=24, visit=None):
    """acn_create_inside_composite of n half-spaces tangent to a unit-ish sphere (a diamond-like polytope, 2n - 1 nodes:
    the upload step compiles an interval-prune program for it).  visit( k, plane ) sees plane k before the composite clones it."""
    planes = []
    for k in range(n):
        p = host.acn_obj_plane_s_create()
        for m in _rot(rng):
            host.acn_obj_rotate(p, C.byref(m))
        host.acn_obj_move(p, A.v3(*plane_normal(p)))   # the plane at distance 1 from the origin, the origin inside
        if visit:
            visit(k, p)
        planes.append(p)
    arr = (C.c_void_p * n)(*planes)
    o = host.acn_create_inside_composite(arr, n)
    for p in planes:
        host.acn_obj_discard(p)
    return o


def balanced_blob(rng, n=20):
    """acn_create_outside_composite of spheres and quadrics (2n - 1 nodes), cut by a ball: programs with ORs and ANDs."""
    parts = []
    for k in range(n):
        kind = ("sphere", "ellipsoid", "sphere", "cone")[k % 4]
        o = make_leaf(kind, rng)
        if kind == "cone":
            ball = host.acn_obj_sphere_s_create(0.5)
            t = host.acn_obj_pair_inside_s_create_pair(o, ball)
            host.acn_obj_discard(o); host.acn_obj_discard(ball)
            o = t
        parts.append(o)
    arr = (C.c_void_p * n)(*parts)
    o = host.acn_create_outside_composite(arr, n)
    for p in parts:
        host.acn_obj_discard(p)
    return o


def tie_compound(rng, groups=8, per=8, shift=0.0, visit=None):
    """(h) A compound of `groups` enveloped sub-compounds of `per` spheres each (>= 64 table entries: the upload step lays
    it out a second time in reverse order), in which sub-compound g + groups / 2 holds exactly the spheres of sub-compound g:
    every leaf exists twice under different parents, so distances tie bit for bit and only the tie rule picks the hit.
    shift > 0: the twins are moved by `shift` along z instead and get envelopes as tight as culling allows -- along z the later
    twin in the table is nearer by less than f3_eps, the case env_behind's margin is for.
    visit( g, k, sphere ) sees sphere k of sub-compound g before it is pushed."""
    half = groups // 2
    spheres = [[(rng.uniform(-1.5, 1.5, 3), float(rng.uniform(0.15, 0.4))) for _ in range(per)] for _ in range(half)]
    top = host.acn_compound_s_create()
    for g in range(groups):
        sub = host.acn_compound_s_create()
        for k, (pos, r) in enumerate(spheres[g % half]):
            s = host.acn_obj_sphere_s_create(r)
            host.acn_obj_set_material(s, b"diffuse")
            if shift and g >= half:
                pos = pos - np.array([0.0, 0.0, shift])
            host.acn_obj_move(s, A.v3(*pos))
            if shift:   # just wide enough for the upload step to call it bounding (culling on, simple_compound_hit)
                host.acn_obj_set_envelope(s, A.v3(*pos), r * (1 + 4e-9))
            if visit:
                visit(g, k, s)
            host.acn_compound_s_push(sub, s)
            host.acn_obj_discard(s)
        c = np.mean([p for p, _ in spheres[g % half]], axis=0)
        host.acn_obj_set_envelope(sub, A.v3(*c), float(max(np.linalg.norm(p - c) + r for p, r in spheres[g % half]) * 1.01))
        host.acn_compound_s_push(top, sub)
        host.acn_obj_discard(sub)
    # a compound without an envelope pushed into a scene contributes its elements; with one it stays one element
    host.acn_obj_set_envelope(top, A.v3(0, 0, 0), 3.2)
    return top


def query_scene(seed=1, trees=6):
    """The synthetic scene of the per-query tests: one light sphere; as matter root elements a leaf of every primitive
    kind, random CSG trees of depth 2 - 6, two balanced composites (>= 32 nodes: interval-prune programs), a complement,
    a scale wrapper and the tie compound.  Returns (scene, roles): roles[k] names root element k of the matter root."""
    rng = np.random.default_rng(seed)
    sc = A.Scene()
    sc.set(image_width=64, image_height=48, gamma=1.0, trace_depth=10, trace_min_intensity=0.03, direct_samples=8,
           path_samples=4, max_path_length=4.0, camera_position=(0, -8, 2), camera_view_direction=(0, 8, -2),
           camera_top_direction=(0, 0, 1), camera_focal_length=3, background_color=(0.3, 0.35, 0.4))
    objs, roles = [], []
    light = host.acn_obj_sphere_s_create(0.7)
    host.acn_obj_set_radiance(light, 25.0)
    host.acn_obj_move(light, A.v3(-1, -2, 7))
    sc.push(light)
    host.acn_obj_discard(light)
    for kind in LEAF_KINDS:
        o = make_leaf(kind, rng)
        host.acn_obj_move(o, A.v3(*rng.uniform(-3, 3, 3)))
        objs.append(o); roles.append(kind)
    for t in range(trees):
        o = random_csg(rng, 2 + t % 5)
        host.acn_obj_move(o, A.v3(*rng.uniform(-3, 3, 3)))
        objs.append(o); roles.append(f"csg{2 + t % 5}")
    o = balanced_polytope(rng)
    host.acn_obj_move(o, A.v3(2.5, 1, 0.5))
    objs.append(o); roles.append("polytope")
    o = balanced_blob(rng)
    host.acn_obj_set_envelope(o, A.v3(0, 0, 0), 2.0)
    host.acn_obj_move(o, A.v3(-2.5, 1, 0))
    objs.append(o); roles.append("blob")
    b = make_leaf("ellipsoid", rng)
    o = host.acn_obj_neg_s_create_neg(b)
    host.acn_obj_discard(b)
    ball = host.acn_obj_sphere_s_create(1.2)
    t = host.acn_obj_pair_inside_s_create_pair(ball, o)
    host.acn_obj_discard(ball); host.acn_obj_discard(o)
    host.acn_obj_move(t, A.v3(0, 3, -1))
    objs.append(t); roles.append("neg")
    inner = random_csg(rng, 2)
    o = host.acn_obj_scale_s_create_scale(inner, A.v3(1.3, 0.7, 1.1))
    host.acn_obj_discard(inner)
    host.acn_obj_move(o, A.v3(0, -3, 1))
    objs.append(o); roles.append("scale")
    o = tie_compound(rng)
    host.acn_obj_move(o, A.v3(0, 0, -3))
    objs.append(o); roles.append("ties")
    o = tie_compound(rng, shift=5e-7)
    host.acn_obj_move(o, A.v3(4, -4, 3))
    objs.append(o); roles.append("near_ties")
    for o in objs:
        sc.push(o)
        host.acn_obj_discard(o)
    return sc, roles


# ---------------------------------------------------------------------------------------------------------------------
# bounding balls and geometry read back from the flat scene

def node_ball(flat, i, default_r=3.0):
    n = flat.node(i)
    if n.flags & 1:
        return np.array(n.env_pos[:]), float(n.env_radius)
    if n.type == ACN_SPHERE:
        return np.array(n.pos[:]), float(n.prm[0])
    return np.array(n.pos[:]), default_r


def leaves_of(flat, i, out=None):
    """indices of the leaf nodes (plane / sphere / squaroid) under node i"""
    out = [] if out is None else out
    n = flat.node(i)
    if n.type in (ACN_PLANE, ACN_SPHERE, ACN_SQUAROID):
        out.append(i)
    elif n.type in (ACN_PAIR_INSIDE, ACN_PAIR_OUTSIDE):
        leaves_of(flat, n.child0, out); leaves_of(flat, n.child1, out)
    elif n.type in (ACN_NEG, ACN_SCALE):
        leaves_of(flat, n.child0, out)
    elif n.type == ACN_COMPOUND:
        for e in flat.elems_of(i):
            leaves_of(flat, e, out)
    return out


def envelopes_of(flat, i, out=None):
    """(centre, radius) of every envelope in the subtree of node i"""
    out = [] if out is None else out
    n = flat.node(i)
    if n.flags & 1:
        out.append((np.array(n.env_pos[:]), float(n.env_radius)))
    if n.type in (ACN_PAIR_INSIDE, ACN_PAIR_OUTSIDE):
        envelopes_of(flat, n.child0, out); envelopes_of(flat, n.child1, out)
    elif n.type in (ACN_NEG, ACN_SCALE):
        envelopes_of(flat, n.child0, out)
    elif n.type == ACN_COMPOUND:
        for e in flat.elems_of(i):
            envelopes_of(flat, e, out)
    return out


def rax(n):
    return np.array(n.rax[:]).reshape(3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# ray classes

def uniform(rng, c, R, n):
    """(a)"""
    o = c + random_dirs(rng, n) * (1.5 * R * rng.random(n) ** (1 / 3))[:, None]
    return RaySet().add(np.concatenate([o, random_dirs(rng, n)], axis=1), "uniform")


def secondary(rng, oracle, flat, rays, a, nor, trix=1.5, n_refract=512):
    """(b) from oracle hits (a, nor) of `rays`: origins at ray_pos( rp, rd, a ) as the renderer computes them, and at
    a + 2 f3_eps (the alternating walk's step); reflected, refracted and hemisphere directions."""
    hit = np.isfinite(a)
    rp, rd, a, nor = rays[hit, :3], rays[hit, 3:], a[hit], unit(nor[hit])
    rs = RaySet()
    if not len(a):
        return rs
    for offs, tag in ((a, "secondary"), (a + 2 * F3_EPS, "secondary_walk")):
        p = ray_pos(rp, rd, offs)
        rs.add(np.concatenate([p, reflection(rd, nor)], axis=1), tag)
        h = random_dirs(rng, len(p))
        rs.add(np.concatenate([p, h], axis=1), tag)
        rs.add(np.concatenate([p, -h], axis=1), tag)
        k = min(n_refract, len(p))
        refr = np.array([oracle.fresnel_refraction(rd[i], -nor[i] if np.dot(rd[i], nor[i]) < 0 else nor[i], trix) for i in range(k)])
        rs.add(np.concatenate([p[:k], refr], axis=1), tag)
    return rs


def perpendicular(rng, d):
    u = np.cross(d, random_dirs(rng, len(d)))
    return unit(u)


def tangent_ball(rng, c, R, n):
    """(c) lines at distance R (1 + k 2^-52) from c, origins 2R before the tangent point and on it"""
    rs = RaySet()
    for k in TANGENT_K:
        d = random_dirs(rng, n)
        u = perpendicular(rng, d)
        foot = c + u * (R * (1 + k * ULP))
        for t0 in (2.0 * R, 0.0):
            rs.add(np.concatenate([foot - d * t0, d], axis=1), "tangent")
    return rs


def squaroid_tangent_lines(node, rng, n, digits=50):
    """(c) tangent lines of the quadric a x^2 + b y^2 + c z^2 + r = 0 (local frame: rax ( p - pos )) built in mpmath:
    a surface point, a direction in its tangent plane, both mapped to the world frame at 50 digits and rounded to fp64;
    the origin lies 1 .. 3 units back along the line.  Returns rays [m, 6] and the exact points [m, 3] (mpf)."""
    import mpmath as mp
    mp.mp.dps = digits
    a, b, c, r = (mp.mpf(float(v)) for v in node.prm[:4])
    M = mp.matrix(rax(node).tolist())
    pos = mp.matrix([float(v) for v in node.pos[:]])
    rays, pts = [], []
    tries = 0
    while len(rays) < n and tries < 20 * n:
        tries += 1
        v = mp.matrix([mp.mpf(float(x)) for x in rng.normal(size=3)])
        if r == 0:   # a cone: a point of the double cone a x^2 + b y^2 + c z^2 = 0 over a random (x, y)
            z2 = -(a * v[0] ** 2 + b * v[1] ** 2) / c
            if z2 <= 0:
                continue
            p = mp.matrix([v[0], v[1], mp.sqrt(z2) * (1 if rng.random() < 0.5 else -1)])
        else:
            q = a * v[0] ** 2 + b * v[1] ** 2 + c * v[2] ** 2
            if q == 0 or (-r / q) <= 0:
                continue
            p = v * mp.sqrt(-r / q)
        if mp.norm(p) > 3:
            continue
        g = mp.matrix([a * p[0], b * p[1], c * p[2]])
        if mp.norm(g) == 0:
            continue
        w = mp.matrix([mp.mpf(float(x)) for x in rng.normal(size=3)])
        t = w - g * (mp.fdot(w, g) / mp.fdot(g, g))
        t = t / mp.norm(t)
        P = pos + M.T * p
        T = M.T * t
        back = mp.mpf(float(rng.uniform(1, 3)))
        O = P - T * back
        d = np.array([float(x) for x in T])
        d = d / np.linalg.norm(d)
        rays.append(np.concatenate([np.array([float(x) for x in O]), d]))
        pts.append(P)
    return np.array(rays).reshape(-1, 6), pts


def dot_dev(n, d):
    """v_mlv in the device's order: ( x x + y y ) + z z"""
    return (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]


def parallel_dir(nor, d, steps=0):
    """d adjusted in its component along the largest |nor| component, one representable step at a time, until
    nor . d == 0 exactly (as the device evaluates it); steps != 0: then on to the first step where nor . d has the sign of
    `steps`, and |steps| - 1 steps further"""
    d = np.array(d, dtype=np.float64)
    k = int(np.argmax(np.abs(nor)))
    d[k] = -(dot_dev(nor, d) - nor[k] * d[k]) / nor[k]
    for _ in range(64):
        v = dot_dev(nor, d)
        if v == 0:
            break
        d[k] = np.nextafter(d[k], -np.inf if (v > 0) == (nor[k] > 0) else np.inf)
    else:
        return None
    if steps:
        up = np.inf if (steps > 0) == (nor[k] > 0) else -np.inf
        for _ in range(64):   # to the first representable tilt of that sign ...
            d[k] = np.nextafter(d[k], up)
            if np.sign(dot_dev(nor, d)) == np.sign(steps):
                break
        else:
            return None
        for _ in range(abs(steps) - 1):   # ... and beyond
            d[k] = np.nextafter(d[k], up)
    return d


PLANE_TILTS = (0, 1, -1, 3, -3)


def plane_parallel(rng, node, n):
    """(c) rays parallel to a plane: nor . rd == 0 exactly, then the smallest representable tilt of either sign and
    two steps beyond it (parallel_dir); origins on the plane and +-f3_eps off it.  Rays come in
    blocks of n per ( tilt in PLANE_TILTS, offset ): the tilt of a ray is PLANE_TILTS[ ( i // n ) // 3 ]."""
    nor = rax(node)[2]
    pos = np.array(node.pos[:])
    rs = RaySet()
    base = []
    while len(base) < n:   # the few directions whose sum steps over 0 without meeting it are drawn again
        d = unit(np.cross(nor, random_dirs(rng, 1)))[0]
        if all(parallel_dir(nor, d, t) is not None for t in PLANE_TILTS):
            base.append(d)
    for tilt in PLANE_TILTS:
        dd = np.array([parallel_dir(nor, d, tilt) for d in base])
        for off in (0.0, F3_EPS, -F3_EPS):
            o = pos + perpendicular(rng, np.tile(nor, (n, 1))) * rng.uniform(0, 2, (n, 1)) + nor * off
            rs.add(np.concatenate([o, dd], axis=1), "tangent")
    return rs


def degenerate(rng, node, n):
    """(d) rays through the apex of a cone (the squaroid's centre) and along the local z axis of cylinders and
    hyperboloids, from both sides and slightly off"""
    M = rax(node)
    pos = np.array(node.pos[:])
    rs = RaySet()
    z = M[2]
    for sgn in (1.0, -1.0):
        o = np.tile(pos - sgn * 3 * z, (n, 1)) + np.outer(rng.choice([0, 1e-12, 1e-7], n), M[0])
        rs.add(np.concatenate([o, np.tile(sgn * z, (n, 1))], axis=1), "degenerate")
    d = random_dirs(rng, n)
    rs.add(np.concatenate([pos - 2 * d, d], axis=1), "degenerate")   # through the centre / apex
    return rs


def far(rng, c, R, n):
    """(e) origins 1e3 .. 1e6 units away, aimed at the ball"""
    D = 10.0 ** rng.uniform(3, 6, n)
    o = c + random_dirs(rng, n) * D[:, None]
    target = c + random_dirs(rng, n) * (R * rng.random(n))[:, None]
    return RaySet().add(np.concatenate([o, unit(target - o)], axis=1), "far")


def envelope_boundary(rng, c, R, n):
    """(f) origins on the envelope sphere and one ulp of the radius in and out"""
    rs = RaySet()
    for f in (1.0, 1 + ULP, 1 - ULP / 2, 1 + 2 * ULP):
        u = random_dirs(rng, n)
        o = c + u * (R * f)
        d = random_dirs(rng, n)
        rs.add(np.concatenate([o, d], axis=1), "envelope")
        rs.add(np.concatenate([o, -u], axis=1), "envelope")
    return rs


def occlusion_limits(a, rng):
    """(g) per oracle distance a: a, nextafter( a, +-inf ), a +- f3_eps, a +- 2 f3_eps, 0, -1, inf -- returned as
    (index into a, limit) pairs"""
    idx, lim = [], []
    fin = np.isfinite(a)
    for k in range(len(a)):
        if fin[k]:
            d = a[k]
            cands = (d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf), d + F3_EPS, d - F3_EPS, d + 2 * F3_EPS, d - 2 * F3_EPS)
        else:
            cands = (0.0, -1.0, np.inf, 1e6)
        for v in cands:
            idx.append(k); lim.append(v)
    for v in (0.0, -1.0, np.inf):
        idx.append(int(rng.integers(0, len(a)))); lim.append(v)
    return np.array(idx), np.array(lim)


def cone_rim(rng, pos, light_pos, light_r, n_dirs):
    """(i) from shading point `pos` towards a spherical light: directions drawn like v_random_sphere_cap in the light's
    frame (sphere_fov: cos_rs = sqrt( 1 - r^2 / L^2 ), cap height h = 1 - cos_rs), including the rim u = 1 and the axis.
    Returns rays [m, 6]."""
    v = light_pos - pos
    L2 = float(np.dot(v, v))
    axis = v / np.sqrt(L2)
    cos_rs = np.sqrt(1.0 - light_r * light_r / L2)
    h = 1 - cos_rs
    # m_con_z frame: any orthonormal frame with z = axis will do for the direction set
    x = unit(np.cross(axis, [0.3, 0.5, 0.8] if abs(axis[2]) > 0.9 else [0, 0, 1]))
    y = np.cross(axis, x)
    u = np.concatenate([[1.0, 1.0, 0.0], rng.random(n_dirs)])
    phi = 2 * np.pi * rng.random(len(u))
    z = 1.0 - u * h
    s = np.sqrt(np.maximum(0.0, 1 - z * z))
    d = np.outer(s * np.sin(phi), x) + np.outer(s * np.cos(phi), y) + np.outer(z, axis)
    d = unit(d)
    return np.concatenate([np.tile(pos, (len(d), 1)), d], axis=1)


def cone_frame_dirs(axis, cyl_hgt, w, eps=(0.0,)):
    """(i) rim directions of a light's sampling cone as k_shade draws them at u = 1 (v_random_sphere_cap: z = 1 - u h,
    scale = sqrt( 1 - z^2 )), in the frame of the device's own axis and cap height (CONE_CULL's outputs): z axis + scale w',
    w' = w turned about the axis by eps (w: a unit vector orthogonal to the axis)"""
    axis = np.asarray(axis, dtype=np.float64)
    z = 1.0 - 1.0 * cyl_hgt
    scale = np.sqrt(1.0 - z * z)
    w = unit(np.asarray(w) - np.dot(w, axis) * axis)
    b = np.cross(axis, w)
    out = []
    for e in eps:
        ww = unit(w + e * b)
        out.append(unit(axis * z + ww * scale))
    return np.array(out)


def cone_tangent_balls(rng, light_c, light_r, c, r, n_planes=3, backs=(0.25, 1.0, 3.0), digits=40):
    """Shading points from which a ball (c, r) -- an element's sphere or envelope -- touches the light's sampling cone from
    outside: points on an internal common tangent line of the light sphere and the ball (built in mpmath, rounded to fp64),
    behind the ball's tangent point, so that the line is a rim generator of the cone and the ball lies just outside it
    (root_cone_cull's cos_phi = cos_sum).  Returns [( point, line direction )]."""
    import mpmath as mp
    mp.mp.dps = digits
    c1 = mp.matrix([mp.mpf(float(v)) for v in light_c]); r1 = mp.mpf(float(light_r))
    c2 = mp.matrix([mp.mpf(float(v)) for v in c]); r2 = mp.mpf(float(r))
    D = c2 - c1
    if mp.norm(D) <= (r1 + r2) * mp.mpf("1.01"):
        return []
    H = (c1 * r2 + c2 * r1) / (r1 + r2)
    e1 = (c1 - H) / mp.norm(c1 - H)
    sb = r1 / mp.norm(c1 - H)
    cb = mp.sqrt(1 - sb * sb)
    out = []
    for _ in range(n_planes):
        q = mp.matrix([mp.mpf(float(v)) for v in rng.normal(size=3)])
        k = mp.matrix([D[1] * q[2] - D[2] * q[1], D[2] * q[0] - D[0] * q[2], D[0] * q[1] - D[1] * q[0]])
        k = k / mp.norm(k)
        e2 = mp.matrix([k[1] * e1[2] - k[2] * e1[1], k[2] * e1[0] - k[0] * e1[2], k[0] * e1[1] - k[1] * e1[0]])
        for sgn in (1, -1):
            d = e1 * cb + e2 * (sgn * sb)
            t2 = -mp.norm(H - c2) * cb   # the ball's tangent point
            for back in backs:
                p = H + d * (t2 - mp.mpf(back) * r2)
                out.append((np.array([float(x) for x in p]), unit(np.array([float(x) for x in d]))))
    return out


def cone_parallel_plane(rng, light_c, light_r, nor, n=6, backs=(0.5, 2.0), digits=40):
    """Shading points from which a rim generator of the light's sampling cone is parallel to a plane of normal `nor`: the
    cone's tangent plane along that generator is parallel to the element plane (root_cone_cull's d_min or d_max = 0).  The
    point lies on a line tangent to the light at T = c +- r nor, with a direction g orthogonal to nor.  Returns
    [( point, g )]."""
    import mpmath as mp
    mp.mp.dps = digits
    c = mp.matrix([mp.mpf(float(v)) for v in light_c])
    nrm = mp.matrix([mp.mpf(float(v)) for v in nor]); nrm = nrm / mp.norm(nrm)
    out = []
    for _ in range(n):
        q = mp.matrix([mp.mpf(float(v)) for v in rng.normal(size=3)])
        g = q - nrm * mp.fdot(q, nrm); g = g / mp.norm(g)
        for sgn in (1, -1):
            T = c + nrm * (sgn * mp.mpf(float(light_r)))
            for back in backs:
                p = T - g * mp.mpf(back)
                out.append((np.array([float(x) for x in p]), unit(np.array([float(x) for x in g]))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# distance objects and rough surfaces (tests/test_rough_distance_cpu.py, tests/test_gpu_rough_distance.py)

ACN_SDF_SPHERE, ACN_SDF_TORUS = 0, 1
ROUGHNESS = (0.002, 0.02, 0.1)   # the values of the lamp scripts
TORUS_ROLES = ("torus", "torus_bare", "torus_short", "rough_torus")   # root elements that are one torus node
DISTANCE_ROLES = ("torus", "torus_bare", "torus_short", "sdf_sphere", "sdf_default")


def _pair_inside(a, b):
    o = host.acn_obj_pair_inside_s_create_pair(a, b)
    host.acn_obj_discard(a); host.acn_obj_discard(b)
    return o


def _neg(a):
    o = host.acn_obj_neg_s_create_neg(a)
    host.acn_obj_discard(a)
    return o


def _scale(a, v):
    o = host.acn_obj_scale_s_create_scale(a, A.v3(*v))
    host.acn_obj_discard(a)
    return o


def _torus(rng, r1=0.5, r2=0.18):
    o = host.acn_obj_torus_create(r1, r2)
    host.acn_obj_set_material(o, b"diffuse")
    return _place(o, rng, spread=0.2)


def rough_distance_scene(seed=2, rough=True):
    """The second query scene: one light sphere; as matter root elements distance objects (tori with and without an envelope,
    with 3 cycles, the sphere function under a scale, the default function; tori as operands of pairs, under NEG and under a
    scale wrapper, in a random tree) and rough surfaces at every place a normal is perturbed (leaves, both operands of a leaf
    pair and the pair, the pair alone, a complemented operand, under a scale wrapper, a random tree, a balanced composite, a
    simple compound with ties between a rough and a smooth twin), and a sphere of negative roughness.  rough=False builds the
    SMOOTH TWIN: the same objects, the same draws and the same node indices, no acn_obj_set_surface_roughness call.
    Returns (scene, roles): roles[k] names root element k of the matter root."""
    rng = np.random.default_rng(seed)
    sc = A.Scene()
    sc.set(image_width=64, image_height=48, gamma=1.0, trace_depth=10, trace_min_intensity=0.03, direct_samples=8,
           path_samples=4, max_path_length=4.0, camera_position=(0, -8, 2), camera_view_direction=(0, 8, -2),
           camera_top_direction=(0, 0, 1), camera_focal_length=3, background_color=(0.3, 0.35, 0.4))
    light = host.acn_obj_sphere_s_create(0.7)
    host.acn_obj_set_radiance(light, 25.0)
    host.acn_obj_move(light, A.v3(-1, -2, 9))
    sc.push(light)
    host.acn_obj_discard(light)
    objs, roles = [], []

    def rgh(o, v):
        if rough:
            host.acn_obj_set_surface_roughness(o, float(v))
        return o

    def add(role, o):
        objs.append(o); roles.append(role)

    def ball(r, at=(0, 0, 0)):
        o = host.acn_obj_sphere_s_create(float(r))
        host.acn_obj_set_material(o, b"diffuse")
        host.acn_obj_move(o, A.v3(*at))
        return o

    # -- distance objects
    add("torus", _torus(rng))
    o = host.acn_obj_distance_s_create()   # assembled by hand: no envelope, not rotated (rays along its axis meet f == 0 exactly)
    assert host.acn_obj_set_distance_function(o, ACN_SDF_TORUS, 0.18 / 0.5) == 0
    host.acn_obj_scale(o, 0.5)
    host.acn_obj_set_material(o, b"diffuse")
    add("torus_bare", _place(o, rng, spread=0.2, rotate=False))
    o = _torus(rng)
    assert host.acn_obj_set_field(o, b"cycles", 3.0) == 1
    add("torus_short", o)
    o = host.acn_obj_distance_s_create()
    assert host.acn_obj_set_distance_function(o, ACN_SDF_SPHERE, 0.0) == 0
    host.acn_obj_scale(o, 0.37)
    host.acn_obj_set_material(o, b"diffuse")
    add("sdf_sphere", _place(o, rng, spread=0.2))
    o = host.acn_obj_distance_s_create()
    host.acn_obj_set_material(o, b"diffuse")
    add("sdf_default", _place(o, rng, spread=0.2))
    add("torus_and_ball", _pair_inside(_torus(rng), ball(0.5, (0.35, 0.1, 0.05))))
    p = host.acn_obj_plane_s_create()
    host.acn_obj_set_material(p, b"diffuse")
    add("torus_minus_half", _pair_inside(_torus(rng), _neg(_place(p, rng, spread=0.1))))
    add("torus_scaled", _scale(_torus(rng), (1.3, 0.7, 1.1)))
    add("torus_hole", _pair_inside(ball(0.6), _neg(_torus(rng))))
    first = [True]

    def torus_leaf(kind, r):
        o = make_leaf(kind, r)   # the draws of the leaf it replaces are made
        if first[0]:
            first[0] = False
            host.acn_obj_discard(o)
            o = host.acn_obj_torus_create(0.5, 0.18)
            host.acn_obj_set_material(o, b"diffuse")
        return o
    add("torus_deep", random_csg(rng, 3, leaf=torus_leaf))

    # -- rough surfaces
    for role, kind, v in (("rough_sphere", "sphere", 0.02), ("rough_plane", "plane", 0.1), ("rough_ellipsoid", "ellipsoid", 0.002),
                          ("rough_cone", "cone", 0.02)):
        add(role, rgh(make_leaf(kind, rng), v))
    add("rough_torus", rgh(_torus(rng), 0.1))
    add("rough_leaf_pair", rgh(_pair_inside(rgh(make_leaf("sphere", rng), 0.1), rgh(make_leaf("plane", rng), 0.002)), 0.02))
    add("rough_pair_only", rgh(_pair_inside(make_leaf("sphere", rng), make_leaf("plane", rng)), 0.1))
    o = host.acn_obj_squaroid_s_create_ellipsoid(1.0, 0.9, 0.8)   # a wide bite out of the ball: its rough wall is what rays see
    host.acn_obj_set_material(o, b"diffuse")
    for m in _rot(rng):
        host.acn_obj_rotate(o, C.byref(m))
    host.acn_obj_move(o, A.v3(0.4, 0.2, 0.1))
    add("rough_neg", _pair_inside(ball(1.0), _neg(rgh(o, 0.02))))
    add("rough_scaled", _scale(rgh(_pair_inside(rgh(make_leaf("sphere", rng), 0.02), rgh(make_leaf("plane", rng), 0.1)), 0.002),
                               (1.3, 0.7, 1.1)))
    # the roughness of the tree's nodes comes from a stream of its own, seeded after the geometry draws above: whatever the tree
    # draws, both twins make the same draws in the same order
    rrng = np.random.default_rng(int(rng.integers(0, 2 ** 62)))

    def every_third(o):
        pick, v = rrng.random() < 1 / 3, ROUGHNESS[int(rrng.integers(0, 3))]
        if pick:
            rgh(o, v)
    add("rough_tree", rgh(random_csg(rng, 4, visit=every_third), 0.02))
    add("rough_polytope", rgh(balanced_polytope(rng, visit=lambda k, p: rgh(p, ROUGHNESS[k % 3]) if k % 3 == 0 else None), 0.02))
    # sphere k of sub-compound g is rough where its bit-identical twin in sub-compound g + groups / 2 is smooth
    add("rough_compound", tie_compound(rng, visit=lambda g, k, s: rgh(s, ROUGHNESS[k % 3]) if (k + (g >= 4)) % 2 else None))
    o = make_leaf("sphere", rng)
    if rough:
        host.acn_obj_set_surface_roughness(o, -0.01)   # the guard is > 0: no perturbation
    add("not_rough", o)

    cols = 6
    for k, o in enumerate(objs):   # a grid, a few units apart
        host.acn_obj_move(o, A.v3(5.0 * (k % cols) - 12.5, 5.0 * (k // cols) - 7.5, 0.0))
        sc.push(o)
        host.acn_obj_discard(o)
    return sc, roles


def nodes_of(flat, i, out=None, scaled=True):
    """indices of every node in the subtree of node i (i first); scaled=False: not those under a scale wrapper"""
    out = [] if out is None else out
    out.append(i)
    n = flat.node(i)
    if n.type in (ACN_PAIR_INSIDE, ACN_PAIR_OUTSIDE):
        nodes_of(flat, n.child0, out, scaled); nodes_of(flat, n.child1, out, scaled)
    elif n.type == ACN_NEG or (n.type == ACN_SCALE and scaled):
        nodes_of(flat, n.child0, out, scaled)
    elif n.type == ACN_COMPOUND:
        for e in flat.elems_of(i):
            nodes_of(flat, e, out, scaled)
    return out


def tori_of(flat, i, scaled=True):
    return [k for k in nodes_of(flat, i, scaled=scaled) if flat.node(k).type == ACN_DISTANCE and flat.node(k).sdf_kind == ACN_SDF_TORUS]


def _torus_frame(node):
    """(pos, rax, inv_scale, r) in longdouble: local = rax ( p - pos ) inv_scale; the local torus has radii 1 and r"""
    L = np.longdouble
    return np.array(node.pos[:], dtype=L), rax(node).astype(L), L(node.prm[0]), L(node.prm[1])


def _torus_world(node, local):
    pos, M, inv, r = _torus_frame(node)
    return pos + (np.asarray(local, dtype=np.longdouble) / inv) @ M


def _rays(o, d, label):
    o = np.asarray(o, dtype=np.float64)
    d = unit(np.asarray(d, dtype=np.float64))
    return RaySet().add(np.concatenate([o, d], axis=1), label)


def torus_tangent(rng, node, n):
    """tangent lines of the exact torus (points, normals and tangent directions in longdouble), shifted along the exact
    normal by k 2^-52 of the torus' size (k in TANGENT_K) and by +-f3_eps and +-10 f3_eps; origins one unit before the tangent
    point and on it"""
    L = np.longdouble
    pos, M, inv, r = _torus_frame(node)
    rs = RaySet()
    size = float((1 + r) / inv)
    for shift in [k * ULP * size for k in TANGENT_K] + [F3_EPS, -F3_EPS, 10 * F3_EPS, -10 * F3_EPS]:
        u, v = rng.uniform(0, 2 * np.pi, n).astype(L), rng.uniform(0, 2 * np.pi, n).astype(L)
        P = np.stack([(1 + r * np.cos(v)) * np.cos(u), (1 + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
        N = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
        Tu = np.stack([-np.sin(u), np.cos(u), np.zeros(n, dtype=L)], axis=1)
        Tv = np.stack([-np.sin(v) * np.cos(u), -np.sin(v) * np.sin(u), np.cos(v)], axis=1)
        w = rng.uniform(0, 2 * np.pi, n).astype(L)
        T = Tu * np.cos(w)[:, None] + Tv * np.sin(w)[:, None]
        Pw, Nw, Tw = _torus_world(node, P), N @ M, T @ M
        foot = Pw + Nw * L(shift)
        for t0 in (1.0, 0.0):
            rs.extend(_rays(foot - Tw * L(t0), Tw, "torus_tangent"))
    return rs


def torus_axis(node):
    """rays along the local z axis through the centre, both ways and from the centre itself (the f == 0 branch of the torus
    function); through the centre in the equatorial plane; parallel to the axis through the tube's centre circle"""
    L = np.longdouble
    pos, M, inv, r = _torus_frame(node)
    z = np.array([0, 0, 1], dtype=L)
    o, d = [], []
    for s in (1, -1):
        for t in (3.0, 1.0, 0.25, 0.0, -0.25):
            o.append(-s * t * z); d.append(s * z)
    for phi in np.linspace(0, 2 * np.pi, 16, endpoint=False):
        e = np.array([np.cos(phi), np.sin(phi), 0], dtype=L)
        for t in (3.0, 0.5, 0.0):
            o.append(e * t); d.append(-e)
        for s in (1, -1):
            o.append(e + s * 3 * z); d.append(-s * z)
            o.append(e); d.append(s * z)
    return _rays(_torus_world(node, np.array(o)), np.array(d) @ M, "torus_axis")


def torus_inside(rng, node, n):
    """origins on the tube's centre circle and at random depths inside the tube, random directions: the inside-out branch"""
    L = np.longdouble
    pos, M, inv, r = _torus_frame(node)
    u, v = rng.uniform(0, 2 * np.pi, n).astype(L), rng.uniform(0, 2 * np.pi, n).astype(L)
    depth = np.where(np.arange(n) % 4 == 0, 0.0, rng.random(n) ** 0.5 * 0.999).astype(L) * r
    P = np.stack([(1 + depth * np.cos(v)) * np.cos(u), (1 + depth * np.cos(v)) * np.sin(u), depth * np.sin(v)], axis=1)
    return _rays(_torus_world(node, P), random_dirs(rng, n), "torus_inside")


def torus_in_hole(rng, node, n):
    """origins outside the tube and inside the envelope of the constructor: in the hole, and off the surface along the exact
    normal by +-f3_eps and +-2 f3_eps (the negative ones just inside); random directions"""
    L = np.longdouble
    pos, M, inv, r = _torus_frame(node)
    h = n // 2
    rad = (rng.random(h) ** 0.5).astype(L) * (1 - r)
    phi = rng.uniform(0, 2 * np.pi, h).astype(L)
    P = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-1, 1, h).astype(L) * r], axis=1)
    rs = _rays(_torus_world(node, P), random_dirs(rng, h), "torus_in_hole")
    m = n - h
    u, v = rng.uniform(0, 2 * np.pi, m).astype(L), rng.uniform(0, 2 * np.pi, m).astype(L)
    off = np.array([F3_EPS, -F3_EPS, 2 * F3_EPS, -2 * F3_EPS], dtype=L)[np.arange(m) % 4] * inv
    q = r + off
    P = np.stack([(1 + q * np.cos(v)) * np.cos(u), (1 + q * np.cos(v)) * np.sin(u), q * np.sin(v)], axis=1)
    return rs.extend(_rays(_torus_world(node, P), random_dirs(rng, m), "torus_in_hole"))


def rough_distance_rays(rng, oracle, flat, e, n=400):
    """the ray set of root element e of rough_distance_scene (about 1500 rays): uniform, secondary, tangents of the bounding
    ball and the envelopes, far and envelope origins, and the four torus classes for every torus under e"""
    node = flat.node(e)
    c, rad = node_ball(flat, e)
    if node.type != ACN_SPHERE and not (node.flags & 1):
        est = oracle.estimate_envelope(flat, e, samples=2000)
        if np.all(np.isfinite(est)) and 0 < est[3] < 10:
            c, rad = np.array(est[:3]), est[3]
    rs = uniform(rng, c, rad, n)
    a, nor, _ = element_hits(oracle, flat, e, rs.rays)
    pick = np.flatnonzero(np.isfinite(a))[:60]
    rs.extend(secondary(rng, oracle, flat, rs.rays[pick], a[pick], nor[pick], n_refract=30))
    rs.extend(tangent_ball(rng, c, rad, 5))
    rs.extend(far(rng, c, rad, 60))
    for ec, er in envelopes_of(flat, e)[:3]:
        rs.extend(envelope_boundary(rng, ec, er, 5))
        rs.extend(tangent_ball(rng, ec, er, 3))
    for t in tori_of(flat, e, scaled=False)[:1]:   # (under a scale wrapper the torus' frame is not the element's)
        tn = flat.node(t)
        rs.extend(torus_tangent(rng, tn, 8))
        rs.extend(torus_axis(tn))
        rs.extend(torus_inside(rng, tn, 120))
        rs.extend(torus_in_hole(rng, tn, 120))
    if node.type == ACN_COMPOUND:   # through leaf centres: the bit-identical twins tie exactly
        cen = np.array([flat.node(l).pos[:] for l in leaves_of(flat, e)[:64]])
        d = random_dirs(rng, len(cen))
        rs.add(np.concatenate([cen - 4 * d, d], axis=1), "ties")
        rs.add(np.concatenate([cen + 4 * d, -d], axis=1), "ties")
    return rs


def element_hits(oracle, flat, e, rays):
    """( a, nor, hit object ) of root element e: compound_s_ray_hit for a compound, obj_ray_hit otherwise"""
    if flat.node(e).type == ACN_COMPOUND:
        return oracle.compound_ray_hits(flat, e, rays)
    a, nor = oracle.obj_ray_hits(flat, e, rays)
    return a, nor, np.full(len(a), e, dtype=np.int64)


class RoughDistanceSets:
    """both scenes flattened, and per role the ray set with the oracle's answers in the rough scene (a, nor, ho) and in the
    smooth twin (ta, tnor).  Built once per test module; nothing in it is written to afterwards."""

    def __init__(self, oracle, seed=2):
        self.scene, self.roles = rough_distance_scene(seed, rough=True)
        self.twin_scene, roles = rough_distance_scene(seed, rough=False)
        assert roles == self.roles
        self.flat, self.twin = self.scene.flatten(), self.twin_scene.flatten()
        self.root = self.flat.c.matter_root
        self.elems = dict(zip(self.roles, self.flat.elems_of(self.root)))
        assert len(self.elems) == len(self.roles) and self.flat.c.n_nodes == self.twin.c.n_nodes
        rng = np.random.default_rng(12)
        self.sets = {}
        for role, e in self.elems.items():
            rs = rough_distance_rays(rng, oracle, self.flat, e)
            a, nor, ho = element_hits(oracle, self.flat, e, rs.rays)
            ta, tnor, _ = element_hits(oracle, self.twin, e, rs.rays)
            for v in (a, nor, ho, ta, tnor, rs.rays):
                v.setflags(write=False)
            self.sets[role] = (rs, a, nor, ho, ta, tnor)

    def rough_nodes(self, role):
        return [k for k in nodes_of(self.flat, self.elems[role]) if self.flat.node(k).surface_roughness > 0]

    def counts(self, a_of=None):
        """per role: rays, finite hits, and hits and misses of the torus_tangent and torus_inside classes, from distances
        a_of[ role ] (default: the oracle's)"""
        out = {}
        for role, (rs, a, nor, ho, ta, tnor) in self.sets.items():
            a = a if a_of is None else a_of[role]
            fin = np.isfinite(a)
            out[role] = {"rays": len(rs), "hits": int(fin.sum())}
            for c in ("torus_tangent", "torus_inside"):
                if (rs.cls == c).any():
                    out[role][c + "_hits"] = int((fin & (rs.cls == c)).sum())
                    out[role][c + "_misses"] = int((~fin & (rs.cls == c)).sum())
        return out

    def check_counts(self, cnt):
        """the tests are not vacuous: >= 100 finite hits per role (torus_short: >= 10); on the tori that are root elements with
        200 cycles >= 10 hits and >= 10 misses of torus_tangent rays and >= 100 torus_inside hits; >= 50 rays leave torus_bare
        with a miss"""
        for role, c in cnt.items():
            print("counts", role, c)
            assert c["hits"] >= (10 if role == "torus_short" else 100), (role, c)
        for role in ("torus", "torus_bare", "rough_torus"):
            assert cnt[role]["torus_tangent_hits"] >= 10 and cnt[role]["torus_tangent_misses"] >= 10, (role, cnt[role])
            assert cnt[role]["torus_inside_hits"] >= 100, (role, cnt[role])
        assert cnt["torus_bare"]["rays"] - cnt["torus_bare"]["hits"] >= 50


def rough_distance_scene_rays(rng, oracle, flat, per=80):
    """rays for the scene-level queries of rough_distance_scene: around every root element, secondary rays of their hits on
    the whole root, tangents of the elements' balls, far origins"""
    root = flat.c.matter_root
    rs = RaySet()
    for e in flat.elems_of(root):
        c, r = node_ball(flat, e, default_r=1.0)
        rs.extend(uniform(rng, c, 1.5 * min(r, 2.0), per))
        rs.extend(tangent_ball(rng, c, min(r, 2.0), 2))
    a, nor, ho = oracle.compound_ray_hits(flat, root, rs.rays)
    pick = np.flatnonzero(np.isfinite(a))[::3]
    rs.extend(secondary(rng, oracle, flat, rs.rays[pick], a[pick], nor[pick], n_refract=60))
    rs.extend(far(rng, np.zeros(3), 8.0, 200))
    return rs


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of the shading stages (tests/test_gpu_stages.py, tests/test_stages_cpu.py)

STAGE_MATTER = ("floor", "wall", "mirror", "chromatic", "water", "glass", "glass_core", "rough", "occluder", "csg", "torus")
STAGE_LIGHTS = ("sphere_light", "plane_light", "pair_light")
# of the torus element: the shading points of the tests lie inside, so every shadow ray enters it.  (The in-line pass of k_shade leaves
# a distance object or a nested compound to the machine whenever the ray hits its envelope; a CSG pair it may still rule out itself,
# by surely_outside or its prune program, so the pair's own envelope does not keep a sample out of the in-line sums.)
STAGE_ENVELOPE = ((0.0, 0.0, 2.0), 12.0)
STAGE_LIMIT_R = 1.0                        # radius of the spheres that path rays meet at max_path_length (stage_limit_cases)


def shade_stage_scene(pair_light=False, direct_samples=200, path_samples=200, limit_spheres=True, **params):
    """Scene A of the stage tests, and with pair_light scene B (a light that is no leaf: k_shade< LEAF_LIGHTS = false >).
    A "diffuse" floor (sigma 0.29), a "diffuse_polished" wall, a perfect mirror, a coloured chromatic 0.7 sphere, coloured glass
    inside water with a core of the glass's index (trix above 1, below 1 and exactly 1 between them), a diffuse sphere with a
    roughness call, a plain sphere in the line of the lights, a torus-and-ball pair, and a torus whose envelope encloses where the
    tests shade: a shadow ray that starts there is never decided in line.  limit_spheres: far outside, the six plain spheres of
    stage_limit_cases, each at max_path_length (or a neighbour of it) along one path sample of a task of scene A.  Lights: a sphere of radius 0.5 with a chess texture, a plane.
    params: acn_params fields set after the scene's own.  Returns (scene, node): node[ name ] after flattening is the node index of
    the object."""
    rng = np.random.default_rng(11)
    sc = A.Scene()
    sc.set(image_width=32, image_height=32, gamma=1.0, trace_depth=22, trace_min_intensity=0.002, direct_samples=direct_samples,
           path_samples=path_samples, max_path_length=30.0, camera_position=(0, -8, 3), camera_view_direction=(0, 8, -2),
           camera_top_direction=(0, 0, 1), camera_focal_length=3, background_color=(0.3, 0.35, 0.4))
    sc.set(**params)
    order = []

    def push(name, o):
        sc.push(o)
        host.acn_obj_discard(o)
        order.append(name)

    def ball(r, at, material, color=None):
        o = host.acn_obj_sphere_s_create(float(r))
        host.acn_obj_set_material(o, material)
        if color is not None:
            host.acn_obj_set_color(o, A.v3(*color))
        host.acn_obj_move(o, A.v3(*at))
        return o

    light = host.acn_obj_sphere_s_create(0.5)
    host.acn_obj_set_radiance(light, 40.0)
    host.acn_obj_set_texture_field_chess(light, A.v3(1.0, 0.9, 0.7), A.v3(0.6, 0.7, 1.0), 3.0)
    host.acn_obj_move(light, A.v3(0.5, -0.5, 5.0))
    push("sphere_light", light)
    light = host.acn_obj_plane_s_create()
    m = host.acn_rotx(180.0)
    host.acn_obj_rotate(light, C.byref(m))                     # faces down
    host.acn_obj_set_color(light, A.v3(0.9, 1.0, 0.8))
    host.acn_obj_set_radiance(light, 300.0)
    host.acn_obj_move(light, A.v3(0.0, 0.0, 9.0))
    push("plane_light", light)
    if pair_light:
        a, b = host.acn_obj_sphere_s_create(0.6), host.acn_obj_plane_s_create()
        light = _pair_inside(a, b)
        host.acn_obj_set_color(light, A.v3(1.0, 0.8, 0.8))
        host.acn_obj_set_radiance(light, 30.0)
        host.acn_obj_move(light, A.v3(-2.0, 1.0, 4.0))
        host.acn_obj_set_envelope(light, A.v3(-2.0, 1.0, 4.0), 0.65)
        push("pair_light", light)

    o = host.acn_obj_plane_s_create()
    host.acn_obj_set_material(o, b"diffuse")
    host.acn_obj_set_color(o, A.v3(0.8, 0.7, 0.6))
    push("floor", o)
    o = host.acn_obj_plane_s_create()
    host.acn_obj_set_material(o, b"diffuse_polished")
    host.acn_obj_set_color(o, A.v3(0.5, 0.8, 0.9))
    m = host.acn_rotx(90.0)
    host.acn_obj_rotate(o, C.byref(m))
    host.acn_obj_move(o, A.v3(0.0, 6.0, 0.0))
    push("wall", o)
    push("mirror", ball(1.0, (-3.0, 0.5, 1.0), b"perfect_mirror"))
    o = ball(0.8, (-1.0, 2.5, 0.8), b"mirror", (0.9, 0.5, 0.3))
    host.acn_obj_set_chromatic_reflectivity(o, 0.7)
    host.acn_obj_set_diffuse_reflectivity(o, 1.0)
    push("chromatic", o)
    push("water", ball(1.2, (3.0, 0.5, 1.2), b"water"))
    o = ball(0.7, (3.0, 0.5, 1.2), b"glass")
    host.acn_obj_set_transparency(o, A.v3(0.6, 0.9, 0.7))
    push("glass", o)
    push("glass_core", ball(0.3, (3.0, 0.5, 1.2), b"glass"))
    o = ball(0.8, (0.5, -2.0, 0.8), b"diffuse", (0.7, 0.8, 0.5))
    host.acn_obj_set_surface_roughness(o, 0.1)
    push("rough", o)
    push("occluder", ball(0.4, (0.4, -0.4, 2.6), b"diffuse"))
    t = host.acn_obj_torus_create(0.5, 0.18)
    host.acn_obj_set_material(t, b"diffuse")
    o = _pair_inside(_place(t, rng, spread=0.1), ball(0.5, (0.3, 0.1, 0.0), b"diffuse"))
    host.acn_obj_move(o, A.v3(-1.5, -1.5, 3.0))
    host.acn_obj_set_envelope(o, A.v3(-1.5, -1.5, 3.0), 1.2)
    push("csg", o)
    t = host.acn_obj_torus_create(0.4, 0.12)
    host.acn_obj_set_material(t, b"diffuse")
    host.acn_obj_move(t, A.v3(1.8, 1.6, 3.2))
    host.acn_obj_set_envelope(t, A.v3(*STAGE_ENVELOPE[0]), STAGE_ENVELOPE[1])
    push("torus", t)
    if limit_spheres:
        for k, case in enumerate(stage_limit_cases()):
            push("limit%d" % k, ball(STAGE_LIMIT_R, case["centre"], b"diffuse"))

    flat = sc.flatten()
    lights, matter = flat.elems_of(flat.c.light_root), flat.elems_of(flat.c.matter_root)
    names_l = [n for n in order if n in STAGE_LIGHTS]
    names_m = [n for n in order if n not in STAGE_LIGHTS]
    assert len(lights) == len(names_l) and len(matter) == len(names_m), (len(lights), len(matter))
    node = dict(zip(names_l, lights))
    node.update(zip(names_m, matter))
    return sc, node


STAGE_N = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 200)   # sample counts of the sample test: around every lane width
_LIMIT_CASES = []


def _sample_point(dtype, prm, fl, pos, nor_up, d, n, depth, T, offs=1.0):
    """a hit record on the floor's material that shades at pos with surface direction nor_up (the side the samples go to), seen along d,
    with n samples per loop"""
    pos, d = np.asarray(pos, dtype=np.float64), unit(np.asarray(d, dtype=np.float64))
    samples = max(prm.direct_samples, prm.path_samples)
    return _hit(dtype, pos - d * offs, d, offs, -unit(np.asarray(nor_up, dtype=np.float64)), -1, fl, depth, (n + 0.5) / samples, T)


def stage_limit_cases():
    """Path hits AT max_path_length.  For scene A with its own sampling parameters: six tasks far outside the scene, and for each a
    plain sphere placed on the ray of one of its path samples so that the oracle's hit distance is max_path_length exactly, its
    predecessor or its successor (the centre is stepped along the ray and by ulps of its coordinates until sphere_ray_hit says so).  Group "inline": the
    ray's line misses the torus' envelope and the sample is bright, so k_shade decides it itself: a child below the limit, a background
    term at and above it.  Group "probe": the line enters the envelope beyond the sphere and the sample is dark (weight *
    diffuse_intensity below trace_min_intensity), so it is an any-hit probe with limit "largest double below max_path_length": not
    written where the sphere is hit below the limit, written at and above it.  The draws of a task depend on its position and normal
    alone, so the cases are found on the scene without the spheres.  Returns dicts: hit (the record), j, target, group, kind, centre."""
    if _LIMIT_CASES:
        return _LIMIT_CASES
    from oracle_binding import Oracle
    import shade_model as M
    oracle = Oracle()
    sc, node = shade_stage_scene(limit_spheres=False)
    flat = sc.flatten()
    prm = flat.params
    dtype = A.Handle.STAGE_RECORDS["hit"]
    rng = np.random.default_rng(41)
    c_env, r_env = np.array(STAGE_ENVELOPE[0]), STAGE_ENVELOPE[1]
    lim = prm.max_path_length
    targets = (("below", np.nextafter(lim, 0.0)), ("at", lim), ("above", np.nextafter(lim, np.inf)))
    kinds = {("inline", "below"): "child", ("inline", "at"): "bsum", ("inline", "above"): "bsum",
             ("probe", "below"): "none", ("probe", "at"): "probe", ("probe", "above"): "probe"}
    cases = []
    for group in ("inline", "probe"):
        for k, (name, target) in enumerate(targets):
            found = None
            for _ in range(20000):
                if group == "inline":
                    pos = np.array([100.0 + 60.0 * k + rng.uniform(0, 20), 100.0 + rng.uniform(0, 20), 40.0])
                    nor_up, n = np.array([0.0, 0.0, -1.0]), 17
                else:
                    u = unit(rng.normal(size=3) + np.array([0.0, 0.0, 1.5]))
                    # the three cases look from different sides, all from above the plane light: of their direct samples the plane's
                    # miss it and the sphere's enter the envelope, so none is decided in line
                    u = unit(np.array([u[0] + 2.0 * (k - 1), u[1], abs(u[2]) + 1.0]))
                    pos = c_env + u * 45.0
                    t = unit(np.cross(u, rng.normal(size=3)))
                    nor_up, n = unit(t - u * 0.03), 5
                t2 = unit(np.cross(nor_up, rng.normal(size=3)))
                hit = _sample_point(dtype, prm, node["floor"], pos, nor_up, -nor_up + 0.2 * t2, n, int(prm.trace_depth), rng.uniform(0.3, 1.0, 3))
                rows = oracle.shade_point(flat, M.tap_input(hit))[0]
                pos = M.rows_of(rows, "surface")[0, 1:4]
                for r in M.rows_of(rows, "path"):
                    d = r[2:5]
                    tca = float((c_env - pos) @ d)
                    off2 = float((c_env - pos) @ (c_env - pos)) - tca * tca
                    enters = tca > 0 and off2 < (0.9 * r_env) ** 2
                    clear = tca <= 0 or off2 > (1.1 * r_env) ** 2
                    dark = r[13] < prm.trace_min_intensity
                    if not (r[5] > 0 and r[7] > lim + 2.5) or any(np.linalg.norm(np.cross(c["centre"] - pos, d)) < 1.5 for c in cases):
                        continue
                    if (group == "inline" and clear and not dark) or (group == "probe" and enters and dark):
                        found = (hit, int(r[1]), pos, d)
                        break
                if found:
                    break
            assert found, (group, name)
            hit, j, pos, d = found
            centre = None
            far = lim + STAGE_LIMIT_R
            far += target - oracle.sphere_ray_hit(pos + d * far, STAGE_LIMIT_R, pos, d)[0]      # (the hit routine has its own f3_eps)
            # (the centre's coordinates are coarser than the distance: its neighbours in each coordinate are tried as well)
            for step in range(-40, 40):
                c0 = pos + d * (far + step * 2.0 ** -49)
                for sh in np.ndindex(5, 5, 5):
                    c = c0 + (np.array(sh) - 2) * np.spacing(c0)
                    if oracle.sphere_ray_hit(c, STAGE_LIMIT_R, pos, d)[0] == target:
                        centre = c
                        break
                if centre is not None:
                    break
            assert centre is not None, (group, name)
            cases.append({"hit": hit, "j": j, "target": target, "group": group, "kind": kinds[(group, name)], "centre": centre})
    _LIMIT_CASES.extend(cases)
    return _LIMIT_CASES


def _hit(dtype, p, d, offs, exit_nor, exit_obj, enter_obj, depth, intensity, T):
    r = np.zeros((), dtype=dtype)
    r["p"], r["d"], r["offs"], r["exit_nor"], r["T"], r["intensity"] = p, d, offs, exit_nor, T, intensity
    r["exit_obj"], r["enter_obj"], r["depth"] = exit_obj, enter_obj, depth
    return r


def stage_base_hits(oracle, flat, node, dtype, seed=21):
    """Transition hits of the oracle on rays aimed at every object of the stage scene from outside, and from inside the water, the
    glass and its core: hit records with intensity 1, the scene's trace_depth and a random throughput."""
    rng = np.random.default_rng(seed)
    depth = int(flat.params.trace_depth)
    rays = []
    eye = np.array([0.0, -8.0, 3.0])
    for name in STAGE_MATTER + STAGE_LIGHTS:
        if name not in node:
            continue
        c, r = node_ball(flat, node[name], default_r=2.0)
        c = np.array([0.0, 0.0, 0.0]) if name == "floor" else np.array([0.0, 6.0, 2.0]) if name == "wall" else np.array([0.0, 0.0, 9.0]) if name == "plane_light" else c
        for _ in range(6):
            t = c + rng.uniform(-0.6, 0.6, 3) * min(r, 2.0)
            rays.append(np.concatenate([eye, unit(t - eye)]))
    gc = np.array(list(flat.node(node["glass"]).pos))
    for rad in (0.1, 0.5, 1.0):                       # inside the core, the glass, the water
        for _ in range(8):
            o = gc + unit(rng.normal(size=3)) * rad
            rays.append(np.concatenate([o, unit(rng.normal(size=3))]))
    out = []
    for ry in rays:
        a, nor, ex, en = oracle.trans_hit(flat, ry[:3], ry[3:])
        if a < np.inf:
            out.append(_hit(dtype, ry[:3], ry[3:], a, nor, ex, en, depth, 1.0, rng.uniform(0.2, 1.0, 3)))
    return out


def stage_split_hits(oracle, flat, node, dtype, seed=22):
    """The records of the split test: every base hit under the intensities and depths at which shade_hit's guards turn, the sample
    counts on an integer and one ulp either side, media set by hand (trix above, below and exactly 1), incidence at the normal and
    1e-8 from grazing, offs = 0 on an exit, a point at a light's pos, and dead slots.  pixel = index."""
    rng = np.random.default_rng(seed)
    prm = flat.params
    tmin, depth = prm.trace_min_intensity, int(prm.trace_depth)
    base = stage_base_hits(oracle, flat, node, dtype)
    recs = []

    def add(r, **kw):
        r = r.copy()
        for k, v in kw.items():
            r[k] = v
        recs.append(r)

    intens = (1.0, tmin, np.nextafter(tmin, 0.0), np.nextafter(tmin, 1.0), 0.5)
    depths = (0, 1, 10, 11, 12, depth)
    for k, b in enumerate(base):
        for i in intens:
            for d in (depths if k % 3 == 0 else (depths[(k + int(i * 7)) % 6], depth)):
                add(b, intensity=i, depth=d)
    # direct_samples * diffuse_intensity and path_samples * diffuse_intensity on an integer and one ulp either side (the floor: reflectivity 1)
    floor_hits = [b for b in base if b["enter_obj"] == node["floor"] and b["exit_obj"] < 0]
    assert floor_hits
    for b in floor_hits[:3]:
        for n in (7, 8, 9, 16, 17, 64, 65, 199):
            for samples in (prm.direct_samples, prm.path_samples):
                v = n / samples
                for i in (np.nextafter(v, 0.0), v, np.nextafter(v, 1.0)):
                    add(b, intensity=i)
    # more samples than any class0_min (the 64-lane class begins above 32 or 255, as the upload decides): 256, 257 and 300 of them
    for b in floor_hits[:2]:
        for n in (256, 257, 300):
            add(b, intensity=(n + 0.25) / prm.direct_samples)
    # media by hand: the stage takes any pair of objects
    w, g, gcore = node["water"], node["glass"], node["glass_core"]
    inside = [b for b in base if b["exit_obj"] >= 0]
    assert inside
    for b in inside:
        for ex, en in ((g, w), (w, g), (g, gcore), (gcore, g), (g, -1), (w, -1), (-1, g), (-1, w)):
            add(b, exit_obj=ex, enter_obj=en)
            add(b, exit_obj=ex, enter_obj=en, offs=0.0, p=ray_pos(b["p"], b["d"], b["offs"]))
    # the critical angle inside the glass against water: sin( theta ) * trix = 1, and the direction's component +- 1, 2 ulp
    trix = flat.node(w).refractive_index / flat.node(g).refractive_index
    nor = np.array([0.0, 0.0, 1.0])
    s = 1.0 / trix if trix > 1 else trix          # sin of the critical angle on the dense side
    for ex, en in ((g, w), (w, g)):
        for k in (-2, -1, 0, 1, 2):
            sx = s
            for _ in range(abs(k)):
                sx = np.nextafter(sx, 2.0 if k > 0 else 0.0)
            d = np.array([sx, 0.0, np.sqrt(1.0 - sx * sx)])
            add(_hit(dtype, (3.0, 0.5, 1.2), d, 0.4, nor, ex, en, depth, 1.0, (0.9, 0.8, 0.7)))
    # incidence at the normal (the projection onto the surface is the zero vector) and 1e-8 from grazing
    fl, rg = node["floor"], node["rough"]
    for en in (fl, node["wall"], node["chromatic"]):
        add(_hit(dtype, (0.3, 0.2, 2.0), (0.0, 0.0, -1.0), 2.0, (0.0, 0.0, -1.0), -1, en, depth, 1.0, (0.7, 0.9, 0.8)))
        gz = unit(np.array([1.0, 0.0, -1e-8]))
        add(_hit(dtype, (-1.0, 0.2, 1e-8), gz, 1.0, (0.0, 0.0, -1.0), -1, en, depth, 1.0, (0.7, 0.9, 0.8)))
    # a normal that faces away from the ray (a rough surface's): theta_i above pi / 2
    add(_hit(dtype, (0.5, -4.0, 0.8), (0.0, 1.0, 0.0), 1.2, unit(np.array([0.1, -0.2, 1.0])), -1, rg, depth, 1.0, (1.0, 1.0, 1.0)))
    # a hit on each light, and one at a light's pos exactly (diff_sqr == 0: F3_MAG, which the fixed-point sum clamps)
    for name in STAGE_LIGHTS:
        if name in node:
            lp = np.array(list(flat.node(node[name]).pos))
            add(_hit(dtype, lp, (0.0, 0.0, 1.0), 0.0, (0.0, 0.0, 1.0), -1, node[name], depth, 1.0, (0.5, 0.25, 0.125)))
            add(_hit(dtype, lp - (0.0, 0.0, 2.0), (0.0, 0.0, 1.0), 1.5, (0.0, 0.0, 1.0), -1, node[name], depth, 0.5, (0.5, 0.25, 0.125)))
    out = np.array(recs, dtype=dtype)
    out["pixel"] = np.arange(len(out))
    dead = rng.choice(len(out), len(out) // 20, replace=False)
    out["pixel"][dead] = 0xFFFFFFFF
    return out


def stage_sample_hits(flat, node, dtype, seed=23, oracle=None):
    """The shading points of the sample test as hit records on the floor's material (the tap and the model make the tasks of them;
    neither asks whether the point lies on the floor): every count of STAGE_N for both loops, with and without a path loop, inside
    the CSG envelope and outside it, on and around the light's sphere, at its centre, 1e6 radii away, on both sides of the plane
    light, the surface direction within 1e-9 .. 1e-3 rad of the light's axis, theta_i at pi / 2 and above, theta_i == theta_r for the
    cone's axis, a sphere's distance at max_path_length (stage_limit_cases).  Tasks of more than one sample per loop lie inside the
    torus' envelope, or ("outside") face away from both lights: nothing of them is decided in line but path rays; the in-line direct
    samples are those of "outside_one", one sample per light, the plane light's in line.  With `oracle` the tasks of the split follow
    ("split": every hit record of stage_split_hits that makes a task without Oren-Nayar term, a quarter of the others), so that the sample
    loops also run without the Oren-Nayar term, with carried colours and on the rough sphere's normals.
    Returns (records, labels, expect): expect[ ( task, j ) ] is what stage_limit_cases says path sample j of the task becomes."""
    rng = np.random.default_rng(seed)
    prm = flat.params
    depth, fl = int(prm.trace_depth), node["floor"]
    lp, lr = np.array(list(flat.node(node["sphere_light"]).pos)), flat.node(node["sphere_light"]).prm[0]
    recs, labels = [], []

    def point(label, pos, nor_up, d, n, depth=depth):
        recs.append(_sample_point(dtype, prm, fl, pos, nor_up, d, n, depth, rng.uniform(0.3, 1.0, 3))); labels.append(label)

    k = 0
    for n in STAGE_N:
        for dp in (depth, 12, 10):
            for where in ("inside", "outside"):
                if where == "inside":
                    xy = rng.uniform(-2.5, 2.5, 2)
                    point(where, (xy[0], xy[1], 0.0), (0, 0, 1), (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0), n, dp)
                else:   # a ceiling point: its samples go down to the floor, away from both lights
                    point(where, (rng.uniform(-2, 2), 20.0 + rng.uniform(0, 2), 1.0), (0, 0, -1), (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0), n, dp)
                k += 1
    for _ in range(12):
        point("outside_one", (rng.uniform(-4, 4), 20.0 + rng.uniform(0, 4), 0.0), (0, 0, 1), (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0), 1, 10)
    up = np.array([0.0, 0.0, 1.0])
    for n in (1, 5, 17, 64):
        u = unit(rng.normal(size=3))
        point("far", lp + u * (1e6 * lr), -u, u + 0.3 * unit(np.cross(u, up)), n)
        for label, pos in stage_light_sphere_points(lp, lr).items():
            point(label, pos, (-1, 0, 0), (1.0, 0.3, 0.1), n)
        point("centre", lp, up, -up, n)
        for z in (8.0, 10.0):
            point("plane_side", (0.3, 0.2, z), (0, 0, 1) if z < 9 else (0, 0, -1), (0.1, 0.0, -1.0 if z < 9 else 1.0), n)
        for eps in (1e-9, 1e-6, 1e-3):
            pos = np.array([1.0, 0.5, 0.0])
            ax = unit(lp - pos)
            t = unit(np.cross(ax, up))
            point("axis", pos, ax * np.cos(eps) + t * np.sin(eps), (0.2, 0.1, -1.0), n)
        for th in (np.pi / 2 - 1e-8, np.pi / 2, np.pi / 2 + 1e-8, 2.0):
            point("grazing", (0.5, 0.5, 0.0), up, (np.sin(th), 0.0, -np.cos(th)), n)
        # theta_i == theta_r for the axis of the cone: the ray comes in as the mirror image of the light's direction
        pos = np.array([-0.5, 0.8, 0.0])
        ax = unit(lp - pos)
        point("tie", pos, up, ax - 2 * up * ax[2], n)
    expect = {}
    for case in stage_limit_cases():
        expect[(len(recs), case["j"])] = case
        r = case["hit"].copy()
        r["enter_obj"] = fl                                   # (the floor's node of THIS scene)
        recs.append(r); labels.append("path_limit")
    if oracle is not None:
        import shade_model as M
        k = 0
        for r in stage_split_hits(oracle, flat, node, dtype):
            if r["pixel"] == 0xFFFFFFFF:
                continue
            rows = oracle.shade_point(flat, M.tap_input(r))[0]
            df = M.rows_of(rows, "diffuse")
            if not len(df) or not np.isfinite(df[0, 4]):      # (a NaN theta_i makes NaN weights, and which NaN is no part of the contract)
                continue
            k += 1
            if M.rows_of(rows, "surface")[0, 9] > 0 and k % 4:
                continue
            recs.append(r.copy()); labels.append("split")
    out = np.array(recs, dtype=dtype)
    out["pixel"] = np.arange(len(out))
    return out, np.array(labels, dtype=object), expect


def stage_light_sphere_points(lp, lr):
    """Points whose v_diff_sqr to the light's centre is radius^2 exactly, the double below it and the double above it (sphere_fov turns
    at diff_sqr > radius_sqr): along x the difference 0.5 is exact, and a y offset of 2^-27 adds one ulp of 0.25; below, x steps in by
    2^-53 (four ulps of the square) and y^2 = 3 * 2^-55 brings the sum back up to the neighbour of 0.25."""
    assert lr == 0.5 and lp[0] == 0.5
    return {"on_light": np.array([lp[0] + lr, lp[1], lp[2]]),
            "off_light": np.array([lp[0] + lr, lp[1] + 2.0 ** -27, lp[2]]),
            "in_light": np.array([lp[0] + (lr - 2.0 ** -53), lp[1] + np.sqrt(3 * 2.0 ** -55), lp[2]])}


# ---------------------------------------------------------------------------------------------------------------------
# the input of the walk stage (tests/test_gpu_stage_walk.py, tests/test_stage_walk_cpu.py): "ray" records, pixel = index

WALK_DEPTHS = (1, 2, 10, 11, 12)     # depth 1: every child is a probe; 10 | 11: the boundary of the path loop


def _walk_records(dtype, rays, T, intensity, depth):
    out = np.zeros(len(rays), dtype=dtype)
    out["p"], out["d"], out["T"], out["intensity"], out["depth"] = rays[:, :3], rays[:, 3:], T, intensity, depth
    return out


def _walk_with_dead_slots(rng, recs):
    """5 % dead slots put in at random places (no ray is lost to them), pixel = index, a total that is a multiple of neither 64 nor 256"""
    n_dead = max(len(recs) // 20, 1)
    while (len(recs) + n_dead) % 64 == 0:
        n_dead += 1
    out = np.zeros(len(recs) + n_dead, dtype=recs.dtype)
    dead = np.zeros(len(out), dtype=bool)
    dead[rng.choice(len(out), n_dead, replace=False)] = True
    out[~dead] = recs
    # what a dead slot holds is not read: values the checks of the seam would refuse
    out["depth"][dead], out["intensity"][dead], out["p"][dead] = -7, np.nan, np.inf
    out["pixel"] = np.arange(len(out))
    out["pixel"][dead] = 0xFFFFFFFF
    return out


def walk_camera_rays(prm, pos=None):
    """the rays of sample positions (default: the scene's raster) in plain numpy: the input of the model and of the device alike"""
    import surface_model
    if pos is None:
        pos = A.main_pass_positions(prm.image_width, prm.image_height)
    return surface_model.camera_rays(prm, np.asarray(pos, dtype=np.float64))


def walk_rays_stage_scene(flat, node, dtype, seed=41):
    """Scene A: the camera rays of its raster and 180 rays started inside the water / glass / core nest, with a random throughput in
    [ 0.2, 1 ]; a copy of every eighth of them at each depth of WALK_DEPTHS, and at each intensity trace_min_intensity, the double
    above it and 0.5; dead slots."""
    rng = np.random.default_rng(seed)
    prm = flat.params
    tmin, depth = prm.trace_min_intensity, int(prm.trace_depth)
    rays = [walk_camera_rays(prm)]
    gc = np.array(list(flat.node(node["glass"]).pos))
    for rad in (0.1, 0.5, 1.0):                       # inside the core, the glass, the water
        o = gc + random_dirs(rng, 60) * rad
        rays.append(np.concatenate([o, random_dirs(rng, 60)], axis=1))
    rays = np.concatenate(rays)
    base = _walk_records(dtype, rays, rng.uniform(0.2, 1.0, (len(rays), 3)), 1.0, depth)
    parts = [base]
    for d in WALK_DEPTHS:
        c = base[::8].copy()
        c["depth"] = d
        parts.append(c)
    for i in (tmin, np.nextafter(tmin, 1.0), 0.5):
        c = base[::8].copy()
        c["intensity"] = i
        parts.append(c)
    return _walk_with_dead_slots(rng, np.concatenate(parts))


def walk_scene_wine_glass():
    sc = A.Scene.build("wine_glass", image_width=48, image_height=27, path_samples=64, direct_samples=50)
    return sc, sc.flatten()


def walk_rays_wine_glass(flat, dtype, seed=42):
    """the wine glass: its camera rays as the pipeline starts them (T = 1, intensity 1, the scene's trace_depth), dead slots"""
    rng = np.random.default_rng(seed)
    prm = flat.params
    rays = walk_camera_rays(prm)
    return _walk_with_dead_slots(rng, _walk_records(dtype, rays, 1.0, 1.0, int(prm.trace_depth)))


def walk_small_scene(diffuse_floor=True, **params):
    """A scene of a dozen nodes whose matter root holds a generic compound (a glass lens cut from two spheres, and a mirror sphere
    beside it): small enough that the upload stages its node array in LDS, and with ACN_PRUNE_MIN=1 the lens gets an interval-prune
    program -- the handle then runs k_walk< LDS, PRUNE >.  Beside the compound a mirror sphere, a sphere light, a sky that rays reach;
    diffuse_floor: a diffuse plane under it all (without it no surface of the scene has a diffuse block, and the picture is the sum
    of the walk's own terms)."""
    sc = A.Scene()
    sc.set(image_width=24, image_height=16, gamma=1.0, trace_depth=12, trace_min_intensity=0.01, direct_samples=4, path_samples=2,
           max_path_length=30.0, camera_position=(0.3, -7, 1.5), camera_view_direction=(0, 7, -0.8), camera_top_direction=(0, 0, 1),
           camera_focal_length=2.2, background_color=(0.3, 0.35, 0.4))
    sc.set(**params)

    def ball(r, at, material):
        o = host.acn_obj_sphere_s_create(float(r))
        host.acn_obj_set_material(o, material)
        host.acn_obj_move(o, A.v3(*at))
        return o

    light = host.acn_obj_sphere_s_create(0.5)
    host.acn_obj_set_radiance(light, 20.0)
    host.acn_obj_move(light, A.v3(-1.5, -1.0, 3.5))
    sc.push(light); host.acn_obj_discard(light)
    lens = _pair_inside(ball(1.0, (0.0, 0.0, 1.0), b"glass"), ball(1.0, (0.7, 0.0, 1.0), b"glass"))
    host.acn_obj_set_material(lens, b"glass")
    cmp = host.acn_compound_s_create()
    host.acn_compound_s_push(cmp, lens)
    s2 = ball(0.4, (-0.9, 0.2, 0.6), b"perfect_mirror")
    host.acn_compound_s_push(cmp, s2)
    host.acn_obj_set_envelope(cmp, A.v3(0.0, 0.0, 1.0), 2.5)
    sc.push(cmp)
    for o in (lens, s2, cmp):
        host.acn_obj_discard(o)
    o = ball(0.7, (2.0, 1.0, 0.7), b"perfect_mirror")
    sc.push(o); host.acn_obj_discard(o)
    o = ball(0.5, (-2.2, 0.5, 0.5), b"water")
    sc.push(o); host.acn_obj_discard(o)
    if diffuse_floor:
        o = host.acn_obj_plane_s_create()
        host.acn_obj_set_material(o, b"diffuse")
        host.acn_obj_set_color(o, A.v3(0.8, 0.7, 0.6))
        sc.push(o); host.acn_obj_discard(o)
    return sc, sc.flatten()


def walk_rays_small_scene(flat, dtype, seed=43):
    """the small scene: its camera rays, and as many aimed at the lens and the mirrors from all around; dead slots"""
    rng = np.random.default_rng(seed)
    prm = flat.params
    cam = walk_camera_rays(prm)
    o = np.array([0.3, 0.0, 1.0]) + random_dirs(rng, len(cam)) * 4.0
    o[:, 2] = np.abs(o[:, 2]) + 0.1
    t = np.array([0.3, 0.0, 0.9]) + rng.uniform(-1.2, 1.2, (len(cam), 3))
    rays = np.concatenate([cam, np.concatenate([o, unit(t - o)], axis=1)])
    return _walk_with_dead_slots(rng, _walk_records(dtype, rays, rng.uniform(0.2, 1.0, (len(rays), 3)), 1.0, int(prm.trace_depth)))

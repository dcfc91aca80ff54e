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

"""A CPU model of the surface records (acn_surface_rays, include/actinon_hip.h) built from the oracle as committed.

The hit is the oracle's: trans_hits on the light root and on the matter root, matter winning only if strictly nearer
(src/scene.c:362-382).  The material rules (src/scene.c:432-470) and the FOLLOW rule (the header's) are restated in numpy with
the expression order of src/gmath.c:68-113 and src/vectors.h: products of a dot product are added left to right, nothing is
contracted.  The albedo comes from two places: obj_color restated in numpy (obj_color_model), and -- for hits with an enter
object -- the oracle itself through an emissive copy of the scene (oracle_albedo), which test_surface_cpu.py pins the numpy
form to."""
import os
import tempfile

import numpy as np

import actinon_amd as A

STRIDE = 16
EMITTER, DIFFUSE, CHROMATIC, FRESNEL, TRANSPARENT, LIGHT_ROOT, CUT = 1, 2, 4, 8, 16, 32, 64
F3_EPS = 1e-6
TIE = 1e-9


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def of_length_1(v):
    """v3d_s_of_length( v, 1 ), src/vectors.h:148-154"""
    r_sqr = dot(v, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r_sqr > 0, 1.0 / np.sqrt(r_sqr), 0.0)
    return np.where((np.abs(r_sqr - 1.0) < 1e-8)[:, None], v, v * f[:, None])


def reflection(d, n):
    """v3d_s_reflection, src/vectors.h:238-241"""
    return of_length_1(d - n * (2.0 * dot(d, n))[:, None])


def fresnel_reflectance(d, n, trix):
    """src/gmath.c:68-93"""
    c = dot(d, n)
    with np.errstate(divide="ignore"):
        f = np.where(c < 0, trix, 1.0 / trix)
    ca = np.abs(c)
    ca = np.where(ca > 1.0, 1.0, ca)
    sa = np.sqrt(1.0 - ca * ca)
    st = sa * f
    with np.errstate(invalid="ignore", divide="ignore"):
        ct = np.sqrt(1.0 - st * st)
        rs = (f * ca - ct) / (f * ca + ct)
        rp = (f * ct - ca) / (f * ct + ca)
        refl = (rs * rs + rp * rp) * 0.5
    return np.where(st < 1, refl, 1.0)


def refraction(d, n, trix):
    """src/gmath.c:95-113"""
    c = dot(d, n)
    with np.errstate(divide="ignore"):
        f = np.where(c < 0, trix, 1.0 / trix)
    q = f * f * (1.0 - c * c)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(1.0 - q)
    b = -f * c + np.where(c > 0, s, -s)
    out = d * f[:, None] + n * b[:, None]
    return np.where((q < 1.0)[:, None], out, d)


def camera_rays(prm, pos):
    """camera_ray (src/scene.c:980-990) in plain numpy: close to the device's rays, not bit-identical (CPU tests only)"""
    W, H = int(prm.image_width), int(prm.image_height)
    unit = 1.0 / (H >> 1)
    ry = np.array(prm.camera_view_direction[:]); ry /= np.sqrt(ry @ ry)
    rz = np.array(prm.camera_top_direction[:]); rz /= np.sqrt(rz @ rz)
    rz = rz - ry * (ry @ rz); rz /= np.sqrt(rz @ rz)
    rx = np.cross(ry, rz)
    z = unit * ((H >> 1) - pos[:, 1]); x = unit * (pos[:, 0] - (W >> 1))
    d = np.stack([x, np.full_like(x, prm.camera_focal_length), z], axis=1)
    d /= np.sqrt((d * d).sum(1))[:, None]
    D = d[:, :1] * rx + d[:, 1:2] * ry + d[:, 2:3] * rz
    P = np.tile(np.array(prm.camera_position[:]), (len(pos), 1))
    return np.concatenate([P, D], axis=1)


def scene_hit(orc, flat, rays):
    """scene_s_trans_hit: a, exit normal, exit object, enter object, hit came from the light root"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    if len(rays) == 0:
        return np.zeros(0), np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
    aL, nL, exL, enL = orc.trans_hits(flat, flat.c.light_root, rays)
    aM, nM, exM, enM = orc.trans_hits(flat, flat.c.matter_root, rays)
    use_m = aM < aL
    a = np.where(use_m, aM, aL)
    n = np.where(use_m[:, None], nM, nL)
    ex = np.where(use_m, exM, exL); en = np.where(use_m, enM, enL)
    miss = ~(a < np.inf)
    ex[miss] = -1; en[miss] = -1
    return a, n, ex, en, ~use_m & ~miss


def materials(flat):
    n = flat.n_nodes
    g = lambda f: np.array([getattr(flat.node(i), f) for i in range(n)], dtype=np.float64)
    tr = np.array([flat.node(i).transparency[:] for i in range(n)], dtype=np.float64)
    return dict(radiance=g("radiance"), ri=g("refractive_index"), fr=g("fresnel_reflectivity"), cr=g("chromatic_reflectivity"),
                dr=g("diffuse_reflectivity"), transp=dot(tr, tr) > 0)


def material_of_hit(m, ex, en):
    """src/scene.c:432-470: emitter, trix, fresnel / chromatic / diffuse reflectivity, transparent; and the kind bits"""
    has_en, has_ex = en >= 0, ex >= 0
    eno = np.where(has_en, en, 0); exo = np.where(has_ex, ex, 0)
    emit = has_en & (m["radiance"][eno] > 0)
    trix = np.where(has_en, m["ri"][eno], 1.0)
    fr = np.where(has_en, ((m["fr"][eno] != 0) & (m["ri"][eno] != 1.0)).astype(np.float64), 0.0)
    cr = np.where(has_en, m["cr"][eno], 0.0)
    dr = np.where(has_en, m["dr"][eno], 0.0)
    tp = np.where(has_en, m["transp"][eno], False)
    with np.errstate(divide="ignore", invalid="ignore"):      # (rows without an exit object divide by node 0's index)
        trix = np.where(has_ex, trix / m["ri"][exo], trix)
    fr = np.where(has_ex, 1.0, fr); cr = np.where(has_ex, 0.0, cr); dr = np.where(has_ex, 0.0, dr); tp = tp | has_ex
    return emit, trix, fr, cr, dr, tp


def kind_bits(emit, fr, cr, dr, tp, light):
    return (EMITTER * emit + DIFFUSE * (dr > 0) + CHROMATIC * (cr > 0) + FRESNEL * (fr > 0) + TRANSPARENT * tp
            + LIGHT_ROOT * light).astype(np.int64)


def obj_color_model(flat, node, pos):
    """obj_color (src/objects.c:411-422) for positions pos on nodes node: the colour, which of the texture's colours it is
    (0 the node's own or a plain texture's, 1 color1, 2 color2), and whether a projected texture coordinate times scale lies
    within 1e-9 of a cell boundary."""
    node = np.asarray(node, dtype=np.int64)
    out = np.zeros((len(node), 3)); which = np.zeros(len(node), np.int64); edge = np.zeros(len(node), bool)
    for nd in np.unique(node):
        sel = node == nd
        o = flat.node(int(nd))
        if o.texture < 0:
            out[sel] = o.color[:]
            continue
        t = flat.c.textures[o.texture]
        if t.kind == 0:
            out[sel] = t.color1[:]
            continue
        p = pos[sel]
        px = np.zeros(len(p)); py = np.zeros(len(p))
        rax = np.array(o.rax[:]).reshape(3, 3)
        opos = np.array(o.pos[:])[None, :]
        if o.type == A.abi.ACN_PLANE:
            q = p - opos
            px = dot(q, rax[0][None, :]); py = dot(q, rax[1][None, :])
        elif o.type == A.abi.ACN_SPHERE:
            q = of_length_1(p - opos)
            x = dot(q, rax[0][None, :]); y = dot(q, np.cross(rax[2], rax[0])[None, :]); z = np.clip(dot(q, rax[2][None, :]), -1, 1)
            px = np.arctan2(x, y); py = np.arcsin(z)
        sx, sy = px * t.scale, py * t.scale
        xi = np.rint(sx).astype(np.int64); yi = np.rint(sy).astype(np.int64)
        one = ((xi ^ yi) & 1) != 0
        out[sel] = np.where(one[:, None], np.array(t.color1[:])[None, :], np.array(t.color2[:])[None, :])
        which[sel] = np.where(one, 1, 2)
        edge[sel] = (np.abs(np.abs(sx - np.floor(sx)) - 0.5) < 1e-9) | (np.abs(np.abs(sy - np.floor(sy)) - 0.5) < 1e-9)
    return out, which, edge


def colours_of(flat, node):
    """the colours obj_color can return for node: [ own / plain ] or [ color1, color2 ]"""
    o = flat.node(int(node))
    if o.texture < 0:
        return [np.array(o.color[:])]
    t = flat.c.textures[o.texture]
    if t.kind == 0:
        return [np.array(t.color1[:])]
    return [np.array(t.color1[:]), np.array(t.color2[:])]


def emissive_copy(flat):
    """the same scene with radiance 1 on every node: scene_s_lum then returns obj_color( enter_obj, pos ) / |pos - enter_obj.pos|^2
    for every hit that has an enter object (src/scene.c:432-436)"""
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "f.npz")
        flat.save(p)
        f = A.Flat.load(p)
    for i in range(f.n_nodes):
        f._nodes[i].radiance = 1.0
    return f


def oracle_albedo(orc, flat, pos_xy, en, hit_pos):
    """The oracle's obj_color( enter_obj, pos ) at the first hit of the camera rays of pos_xy (rows with en >= 0; others NaN)."""
    fe = emissive_copy(flat)
    lum = orc.render_positions(fe, pos_xy, linear=True)
    npos = np.array([flat.node(int(e)).pos[:] if e >= 0 else (np.nan,) * 3 for e in en]).reshape(-1, 3)
    dsq = ((hit_pos - npos) ** 2).sum(1)
    return lum * dsq[:, None]


def exact_colour(flat, node, approx, tol=1e-9):
    """the colour of node's texture (or the node's own) that approx identifies within tol, and its index; raises if none or two do"""
    out = np.zeros((len(node), 3)); which = np.zeros(len(node), np.int64)
    for i, (nd, ap) in enumerate(zip(node, approx)):
        cands = colours_of(flat, nd)
        ok = [k for k, c in enumerate(cands) if np.abs(c - ap).max() <= tol]
        assert len(ok) == 1, (i, int(nd), ap, cands)
        out[i] = cands[ok[0]]
        which[i] = ok[0] + (1 if len(cands) == 2 else 0)
    return out, which


def blank(n):
    rec = np.zeros((n, STRIDE))
    rec[:, 0] = np.inf; rec[:, 7] = -1; rec[:, 8] = -1; rec[:, 14] = 1.0
    return rec


def write_hit(flat, rec, idx, dist, p, d, a, nor, ex, en, kind, hops, weight):
    pos = p + d * a[:, None]
    s = np.where(en >= 0, en, ex)
    col, _, edge = obj_color_model(flat, s, pos)
    rec[idx, 0] = dist; rec[idx, 1:4] = pos; rec[idx, 4:7] = nor; rec[idx, 7] = en; rec[idx, 8] = ex
    rec[idx, 9:12] = col; rec[idx, 12] = kind; rec[idx, 13] = hops; rec[idx, 14] = weight
    return edge


def first_hit(orc, flat, rays):
    """records of ACN_SURF_FIRST_HIT; second value: rows whose albedo lies near a texture cell boundary"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6).copy()
    rays[:, 3:] = of_length_1(rays[:, 3:])
    n = len(rays)
    rec = blank(n)
    edge = np.zeros(n, bool)
    a, nor, ex, en, light = scene_hit(orc, flat, rays)
    k = np.flatnonzero(a < np.inf)
    emit, trix, fr, cr, dr, tp = material_of_hit(materials(flat), ex[k], en[k])
    edge[k] = write_hit(flat, rec, k, a[k], rays[k, :3], rays[k, 3:], a[k], nor[k], ex[k], en[k],
                        kind_bits(emit, fr, cr, dr, tp, light[k]), 0, 1.0)
    return rec, edge


def follow(orc, flat, rays):
    """records of ACN_SURF_FOLLOW; second value: rows where the two largest shares came within TIE of each other at some hop"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6).copy()
    rays[:, 3:] = of_length_1(rays[:, 3:])
    n = len(rays)
    m = materials(flat)
    max_hits = max(int(flat.params.trace_depth), 1)
    rec = blank(n)
    live = np.ones(n, bool)
    hops = np.zeros(n, np.int64); weight = np.ones(n); dist = np.zeros(n)
    near_tie = np.zeros(n, bool)
    r = rays
    while live.any():
        idx = np.flatnonzero(live)
        a, nor, ex, en, light = scene_hit(orc, flat, r[idx])
        dist[idx] = dist[idx] + a
        miss = ~(a < np.inf)
        mi = idx[miss]
        rec[mi, 13] = hops[mi]; rec[mi, 14] = weight[mi]
        live[mi] = False
        k = ~miss
        idx, a, nor, ex, en, light = idx[k], a[k], nor[k], ex[k], en[k], light[k]
        if len(idx) == 0:
            continue
        p, d = r[idx, :3], r[idx, 3:]
        emit, trix, fr, cr, dr, tp = material_of_hit(m, ex, en)
        kind = kind_bits(emit, fr, cr, dr, tp, light)
        refl = np.where(~emit & (fr > 0), fresnel_reflectance(d, nor, trix) * fr, 0.0)
        rest = 1.0 - refl
        w0 = refl
        w1 = cr * rest; rest = rest * (1.0 - cr)
        w2 = dr * rest; rest = rest * (1.0 - dr)
        w3 = np.where(tp, rest, 0.0)
        w = np.stack([w0, w1, w2, w3], axis=1)
        best = np.argmax(w, axis=1)            # the first maximum: the lowest index on a tie
        srt = np.sort(w, axis=1)
        bw = srt[:, 3]
        near_tie[idx] |= ~emit & (bw > 0) & ((bw - srt[:, 2]) < TIE)
        go = ~emit & (bw > 0) & (best != 2)
        cut = go & (hops[idx] + 1 >= max_hits)
        kind = kind + CUT * cut
        cont = go & ~cut
        s = ~cont
        write_hit(flat, rec, idx[s], dist[idx[s]], p[s], d[s], a[s], nor[s], ex[s], en[s], kind[s], hops[idx[s]], weight[idx[s]])
        live[idx[s]] = False
        gi = idx[cont]
        if len(gi):
            pc, dc, ac, nc, tc, bc = p[cont], d[cont], a[cont], nor[cont], trix[cont], best[cont]
            nd = np.where((bc == 3)[:, None], refraction(dc, nc, tc), reflection(dc, nc))
            offs = np.where(bc == 3, ac + 2.0 * F3_EPS, ac)
            r[gi, :3] = pc + dc * offs[:, None]
            r[gi, 3:] = nd
            weight[gi] = weight[gi] * bw[cont]
            hops[gi] += 1
    return rec, near_tie

"""The hard-ray kernels resume k_shade's in-line pass over the matter root instead of redoing it (acn_device.h: the
fast-path forms, root_occluded_rec, root_trans_hit_rec).  Here, ray by ray through the test seam acn_query_rays
(run on the MI355X: -m gpu):

  OCCLUDED  o[1] root_occluded_fast, o[3] its candidate word, o[2] the occlusion test resumed over that word where
            o[1] == 2 -- which must be o[0], the answer of the full test;
  TRANS     columns 6 .. 11: the transition fold resumed over the word of root_trans_hit_fast (o[13]) where that says
            hard -- which must be columns 0 .. 5, the full fold, bit for bit.

Candidate word: bit i < 29: the root element at position i; bit 29 (the tail): some element at a position >= 29."""
import os
from collections import Counter

import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import scenes_util as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POSITIONS = 29
TAIL = 1 << POSITIONS
SCENES = ["wine_glass", "paraffin_lamp", "hanging_lamp", "paraffin_lamp_on_ledge", "textured"]
# Roots with machine elements at positions >= 29: hard answers with the tail bit set must occur, and where the elements
# beyond can all be ruled out, hard answers with the bit clear.  (paraffin_lamp's root has 8 elements -- its tail bit can
# never be set, which is asserted instead; paraffin_lamp_on_ledge, 110 elements, is the second lamp fixture with a long root.)
LONG_ROOTS = ("hanging_lamp", "paraffin_lamp_on_ledge")
# ( scene, scene view ) in which the clear state is reachable.  Both long roots hold CSG objects without an envelope at
# positions >= 29 (hanging_lamp: the burner, element 58; the ledge scene: the ledge and two more); only a prune program can
# rule those out -- surely_outside gives up below three levels -- so the plain view of hanging_lamp sets the tail bit on every
# hard answer, and so does either view of the ledge scene for every ray tried here.
CLEAR_TAIL = {("hanging_lamp", True)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def load(name):
    if name == "wine_glass":
        return A.Scene.build("wine_glass", image_width=96, image_height=54).flatten()
    if name == "textured":
        return S.build("textured")[1]
    return A.Flat.load(os.path.join(HERE, "golden", "scenes", name + ".npz"))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def env_enters(node, rays):
    """env_ray_hits (acn_dev_leaves.h) in the device's order of operations; True where the node has no envelope"""
    if not (node.flags & 1):
        return np.ones(len(rays), bool)
    c, r = np.array(node.env_pos[:]), float(node.env_radius)
    p = rays[:, :3] - c
    d = rays[:, 3:]
    s = (p[:, 0] * d[:, 0] + p[:, 1] * d[:, 1]) + p[:, 2] * d[:, 2]
    q = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) - r * r
    return ~(s * s < q) & ((s < 0) | (q < 0))


def element_hits(oracle, flat, e, rays):
    if flat.node(e).type == R.ACN_COMPOUND:
        return oracle.compound_ray_hits(flat, e, rays)[0]
    return oracle.obj_ray_hits(flat, e, rays)[0]


def scene_ball(flat, els):
    """a ball around everything of the root that has an extent (planes have none)"""
    balls = [R.node_ball(flat, e) for e in els if (flat.node(e).flags & 1) or flat.node(e).type == R.ACN_SPHERE]
    c = np.mean([b[0] for b in balls], axis=0)
    return c, max(float(np.linalg.norm(b[0] - c)) + b[1] for b in balls)


def scene_rays(rng, oracle, flat, n=1200):
    """the ray classes of the scene queries of test_gpu_queries.py, around this scene's objects; rays aimed at the
    envelopes of the first and of the last root element that has one (the tail bit's two states)"""
    root = flat.c.matter_root
    els = flat.elems_of(root)
    c, rad = scene_ball(flat, els)
    rs = R.uniform(rng, c, rad, n)
    a, nor, ho = oracle.compound_ray_hits(flat, root, rs.rays)
    rs.extend(R.secondary(rng, oracle, flat, rs.rays, a, nor, n_refract=100))
    enveloped = [e for e in els if flat.node(e).flags & 1]
    for e in els:
        ec, er = R.node_ball(flat, e, default_r=1.0)
        rs.extend(R.tangent_ball(rng, ec, er, 4))
    for e in (enveloped[0], enveloped[-1]):
        ec, er = R.node_ball(flat, e)
        o = c + R.random_dirs(rng, 150) * (1.5 * rad)
        t = ec + R.random_dirs(rng, 150) * (er * rng.random(150)[:, None])
        rs.add(np.concatenate([o, R.unit(t - o)], axis=1), "aimed")
        rs.extend(R.envelope_boundary(rng, ec, er, 6))
    # short-range rays at single elements of the first positions, from close by: they meet little else of the scene, so
    # whatever lies at the positions a word cannot name is ruled out for most of them (the tail bit's clear state)
    for e in [e for e in els[:POSITIONS] if flat.node(e).flags & 1][:16]:
        ec, er = R.node_ball(flat, e)
        o = ec + R.random_dirs(rng, 40) * (er * rng.uniform(1.5, 4.0, 40)[:, None])
        t = ec + R.random_dirs(rng, 40) * (er * rng.random(40)[:, None])
        rs.add(np.concatenate([o, R.unit(t - o)], axis=1), "close")
    rs.extend(R.far(rng, c, rad, 100))
    return rs


def cone_rays(rng, oracle, flat, h, pts, n_dirs=10):
    """shadow rays as k_shade's direct-light loop casts them from `pts` at the first light, drawn in the device's own
    frame (CONE_CULL returns axis and cap height), with the skip mask of their point and the light's distance as limit"""
    light = flat.elems_of(flat.c.light_root)[0]
    g = h.query_rays("cone_cull", light, np.concatenate([pts, np.tile([0, 0, 1.0], (len(pts), 1))], axis=1))
    masks = g[:, 0].copy().view(np.uint64)
    rays, skip = [], []
    for k, p in enumerate(pts):
        axis, cyl = g[k, 1:4], g[k, 5]
        if not (g[k, 4] > 1e-6):
            continue
        x = R.unit(np.cross(axis, [0.3, 0.5, 0.8] if abs(axis[2]) > 0.9 else [0, 0, 1.0]))
        y = np.cross(axis, x)
        u = np.concatenate([[1.0, 0.0], rng.random(n_dirs)])
        phi = 2 * np.pi * rng.random(len(u))
        z = 1.0 - u * cyl
        s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        d = R.unit(np.outer(s * np.sin(phi), x) + np.outer(s * np.cos(phi), y) + np.outer(z, axis))
        rays.append(np.concatenate([np.tile(p, (len(d), 1)), d], axis=1))
        skip += [int(masks[k])] * len(d)
    rays = np.concatenate(rays)
    skip = np.array(skip, dtype=np.uint64)
    la = oracle.obj_ray_hits(flat, light, rays)[0]
    ok = np.isfinite(la)
    return rays[ok], la[ok], skip[ok]


def named(word, k):
    """rays whose candidate word names position k"""
    w = word.astype(np.uint64)
    return ((w >> np.uint64(min(k, POSITIONS))) & np.uint64(1)) != 0


@pytest.fixture(scope="module", params=SCENES)
def scene(request, oracle):
    name = request.param
    flat = load(name)
    root = flat.c.matter_root
    els = flat.elems_of(root)
    rng = np.random.default_rng(17)
    rs = scene_rays(rng, oracle, flat)
    a = oracle.compound_ray_hits(flat, root, rs.rays)[0]
    idx, lim = R.occlusion_limits(a, rng)
    close = np.flatnonzero(rs.cls[idx] == "close")   # a few thousand occlusion queries: every close-range one, a sample of the rest
    rest = np.flatnonzero(rs.cls[idx] != "close")
    keep = np.concatenate([close, rest[rng.permutation(len(rest))[:5000]]])
    idx, lim = idx[keep], lim[keep]
    per_element = np.array([element_hits(oracle, flat, e, rs.rays) for e in els])    # [ element ][ ray ]
    h = A.Handle(flat)
    info = h.query_rays("elements", root, n=len(els))
    assert [int(v) for v in info[:, 0]] == list(els)
    staged = info[0, 3] != 0
    yield dict(name=name, flat=flat, root=root, els=els, rs=rs, a=a, idx=idx, lim=lim, per_element=per_element, h=h,
               info=info, placements=[True, False] if staged else [False], rng=rng)
    h.close()


def machine_positions(info, prune):
    """root positions whose element goes through the machines in the scene view at hand (the plain view has no in-line
    simple compounds)"""
    inline = 7 if prune else 3   # ACN_Q_EL_FAST | ACN_Q_EL_LEAF_PAIR ( | ACN_Q_EL_SIMPLE_COMPOUND )
    return [k for k in range(len(info)) if not (int(info[k, 1]) & inline)]


def check_occluded(s, o, machine, what):
    """the equalities of one OCCLUDED result set; returns the indices of the hard answers"""
    hard = o[:, 1] == 2
    assert np.array_equal(o[hard, 2], o[hard, 0]), f"{what}: the resumed occlusion test differs from the full one on {int((o[hard, 2] != o[hard, 0]).sum())} rays"
    assert np.isnan(o[~hard, 2]).all(), what
    word = o[:, 3]
    assert (word[~hard] == 0).all() and (word[hard] != 0).all(), what
    assert (word == np.floor(word)).all() and (word < 2 * TAIL).all(), what
    for k in range(POSITIONS):
        if k not in machine:
            assert not named(word, k).any(), f"{what}: a word names position {k}, which is no machine element"
    if not any(k >= POSITIONS for k in machine):
        assert not named(word, POSITIONS).any(), f"{what}: tail bit without a machine element at a position >= {POSITIONS}"
    return hard


def test_resumed_occlusion_equals_the_full_test(scene, oracle):
    s = scene
    h, rs, idx, lim = s["h"], s["rs"], s["idx"], s["lim"]
    rays = rs.rays[idx]
    want = s["a"][idx] <= lim
    counts = Counter()
    for prune in (True, False):
        machine = machine_positions(s["info"], prune)
        # what the CPU knows for sure (oracle hits per element, numpy envelope test): with no in-line element occluding,
        #   a machine element at a position >= 29 that hits within the limit must leave the tail bit set;
        #   one at a position < 29 that does, while the ray misses the envelope of every one beyond, must leave it clear
        #   (a CSG element beyond that has no envelope is ruled out by surely_outside / prune_run alone: asked of the device)
        inline_occ = np.zeros(len(rays), bool)
        early_hit = np.zeros(len(rays), bool)
        late_hit = np.zeros(len(rays), bool)
        late_enter = np.zeros(len(rays), bool)
        bare = []
        for k, e in enumerate(s["els"]):
            hit = s["per_element"][k][idx] <= lim
            node = s["flat"].node(e)
            if k not in machine:
                inline_occ |= hit
            elif k < POSITIONS:
                early_hit |= hit
            else:
                late_hit |= hit
                if (node.flags & 1) or node.type in (R.ACN_COMPOUND, R.ACN_DISTANCE):
                    late_enter |= env_enters(node, rays)
                else:
                    bare.append(e)
        long_root = any(k >= POSITIONS for k in machine)
        assert long_root == (s["name"] in LONG_ROOTS) or not prune, (s["name"], machine)
        sure_tail = want & ~inline_occ & late_hit
        for lds in s["placements"]:
            what = f"{s['name']} lds={lds} prune={prune}"
            sure_clear = want & ~inline_occ & early_hit & ~late_enter
            for e in bare:
                p = h.query_rays("prune", e, rays, limits=lim, lds=lds, prune=prune)
                sure_clear &= (p[:, 0] != 0) | (p[:, 1] != 0)
            if long_root:
                assert sure_tail.sum() > 0, what
            if (s["name"], prune) in CLEAR_TAIL:
                assert sure_clear.sum() > 0, what
            o = h.query_rays("occluded", s["root"], rays, limits=lim, lds=lds, prune=prune)
            assert np.array_equal(o[:, 0] != 0, want), what
            hard = check_occluded(s, o, machine, what)
            assert hard.sum() > 0, f"{what}: no hard answers"
            assert hard[sure_tail | sure_clear].all(), what
            assert named(o[sure_tail, 3], POSITIONS).all(), f"{what}: tail bit clear with a hit beyond position {POSITIONS}"
            assert not named(o[sure_clear, 3], POSITIONS).any(), f"{what}: tail bit set with every envelope beyond position {POSITIONS} missed"
            for k in machine:   # an element that hits within the limit is a candidate
                must = hard & (s["per_element"][k][idx] <= lim)
                assert named(o[must, 3], k).all(), f"{what}: the word leaves out position {k}, which occludes"
            counts["hard"] += int(hard.sum())
            counts["tail"] += int(named(o[hard, 3], POSITIONS).sum())
            # the answers do not depend on which rays share a wave
            perm = s["rng"].permutation(len(rays))
            o2 = h.query_rays("occluded", s["root"], rays[perm], limits=lim[perm], lds=lds, prune=prune)
            assert np.array_equal(bits(o2[:, :4]), bits(o[perm, :4])), f"{what}: answers change with the rays' order"
    print(s["name"], "occlusion queries", len(rays), dict(counts))


def test_resumed_occlusion_with_cone_cull_masks(scene, oracle):
    """k_shade's arrangement: shadow rays of a shading point's light cone, with the point's skip mask"""
    s = scene
    h, rs, flat = s["h"], s["rs"], s["flat"]
    fin = np.flatnonzero(np.isfinite(s["a"]) & (s["a"] > 0) & (s["a"] < 1e3))
    pick = fin[s["rng"].permutation(len(fin))[:250]]
    pts = R.ray_pos(rs.rays[pick, :3], rs.rays[pick, 3:], s["a"][pick])
    rays, la, skip = cone_rays(s["rng"], oracle, flat, h, pts)
    want = oracle.compound_ray_hits(flat, s["root"], rays)[0] <= la
    n_hard = 0
    for prune in (True, False):
        machine = machine_positions(s["info"], prune)
        for lds in s["placements"]:
            what = f"{s['name']} cone cull lds={lds} prune={prune}"
            o = h.query_rays("occluded", s["root"], rays, limits=la, skip=skip, lds=lds, prune=prune)
            assert np.array_equal(o[:, 0] != 0, want), what
            assert not (((o[:, 1] == 0) & want) | ((o[:, 1] == 1) & ~want)).any(), what
            hard = check_occluded(s, o, machine, what)
            n_hard += int(hard.sum())
            perm = s["rng"].permutation(len(rays))
            o2 = h.query_rays("occluded", s["root"], rays[perm], limits=la[perm], skip=skip[perm], lds=lds, prune=prune)
            assert np.array_equal(bits(o2[:, :4]), bits(o[perm, :4])), f"{what}: answers change with the rays' order"
    print(s["name"], "cone rays", len(rays), "hard", n_hard, "culled bits", int(sum(bin(int(m)).count("1") for m in skip)))
    assert len(rays) > 500


def test_resumed_transition_fold_equals_the_full_fold(scene, oracle):
    s = scene
    h, rs = s["h"], s["rs"]
    ta, tn, tex, ten = oracle.trans_hits(s["flat"], s["root"], rs.rays)
    fin = np.isfinite(ta)
    n_hard = 0
    for prune in (True, False):
        machine = machine_positions(s["info"], prune)
        for lds in s["placements"]:
            what = f"{s['name']} trans lds={lds} prune={prune}"
            g = h.query_rays("trans", s["root"], rs.rays, lds=lds, prune=prune)
            for off in (0, 6):
                bad = bits(g[:, off]) != bits(ta)
                bad |= fin & (bits(g[:, off + 1:off + 4]) != bits(tn)).any(axis=1)
                bad |= fin & ((g[:, off + 4] != tex) | (g[:, off + 5] != ten))
                assert not bad.any(), f"{what}: columns {off}..{off + 5} differ from the oracle on {int(bad.sum())} rays, first {rs.rays[np.flatnonzero(bad)[0]].tolist()}"
            hard = g[:, 12] != 0
            word = g[:, 13]
            # hard: some machine element is a candidate; the other candidates are in-line elements that hit; every element
            # that hits is a candidate (the fold needs them all)
            assert (word == np.floor(word)).all() and (word[hard] != 0).all() and (word < 2 * TAIL).all(), what
            early_machine = np.zeros(len(rs), bool)
            for k in range(len(s["els"])):
                hits = np.isfinite(s["per_element"][k])
                assert named(word[hard & hits], k).all(), f"{what}: the word leaves out position {k}, which hits"
                if k >= POSITIONS:
                    continue
                if k in machine:
                    early_machine |= named(word, k)
                else:
                    assert hits[named(word, k)].all(), f"{what}: a word names in-line position {k}, which misses"
            assert hard[early_machine].all(), what
            if not any(k >= POSITIONS for k in machine):
                assert np.array_equal(early_machine, hard), what
            n_hard += int(hard.sum())
            perm = s["rng"].permutation(len(rs))
            g2 = h.query_rays("trans", s["root"], rs.rays[perm], lds=lds, prune=prune)
            assert np.array_equal(bits(g2[:, :14]), bits(g[perm, :14])), f"{what}: answers change with the rays' order"
    print(s["name"], "trans rays", len(rs), "hard", n_hard)
    assert n_hard > 0

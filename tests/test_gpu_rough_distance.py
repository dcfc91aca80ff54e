"""Distance objects and rough surfaces on the device, ray by ray against the CPU oracle (run on the MI355X: -m gpu).

tests/test_gpu_queries.py checks every traversal shortcut on a scene without a distance object and without a rough surface.
Here the scene of ray_sets.rough_distance_scene holds both at every place the device treats them: distance_ray_hit as a root
element, as an operand of both machines, under NEG and under a scale wrapper, with 3 and with 200 cycles, with and without an
envelope; roughness_normal at the in-line leaf and leaf-pair operands, the machines' frames and final node, the simple-compound
table, element_hit and the root loops.  The rays aim at the torus' tangents, axis, tube interior and hole.  Every answer is
compared with the oracle bit for bit; tests/test_rough_distance_cpu.py pins the oracle to closed forms."""
from collections import Counter

import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import rough_model as M
from query_checks import VARIANTS, bits, check_trans_and_occlusion, report_mismatch, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def S(oracle):
    return R.RoughDistanceSets(oracle)


@pytest.fixture(scope="module")
def handles(S):
    hs = {"default": upload(S.flat), "prune_min_1": upload(S.flat, ACN_PRUNE_MIN=1), "twin": upload(S.twin)}
    yield hs
    for h in hs.values():
        h.close()


def variants(h, root):
    """VARIANTS, and the LDS placement of the nodes too where the handle stages them"""
    staged = h.query_rays("elements", root, n=1)[0, 3] > 0
    return VARIANTS + ([(True, True), (True, False)] if staged else [])


def simple(S, role):
    return S.flat.node(S.elems[role]).type != R.ACN_COMPOUND


# ---- 1. hits ------------------------------------------------------------------------------------------------------

def test_hits_bit_identical(S, handles):
    """hit_lane, hit_uni and element_hit, both scene views, every element: the oracle's distance bit for bit, its normal
    wherever the distance is finite, and element_hit reports the element"""
    h = handles["default"]
    for role, e in S.elems.items():
        if not simple(S, role):
            continue
        rs, a, nor, ho, ta, tnor = S.sets[role]
        fin = np.isfinite(a)
        for lds, prune in variants(h, S.root):
            for op in ("hit_lane", "hit_uni", "element_hit"):
                g = h.query_rays(op, e, rs.rays, lds=lds, prune=prune)
                bad = bits(g[:, 0]) != bits(a)
                bad |= fin & (bits(g[:, 1:4]) != bits(nor)).any(axis=1)
                if op == "element_hit":
                    bad |= fin & (g[:, 4] != e)
                assert not bad.any(), report_mismatch(f"{op} lds={lds} prune={prune}", role, rs, bad)


# ---- 2. sides -----------------------------------------------------------------------------------------------------

def test_sides_equal_oracle(S, handles, oracle):
    """side_lane and side_uni equal the oracle's obj_side at the ray origins -- those of the torus_axis class lie on the torus'
    axis and on the tube's centre circle, those of torus_inside and torus_in_hole in the tube and f3_eps off its surface -- and
    at the hit points +- f3_eps"""
    h = handles["default"]
    for role, e in S.elems.items():
        if not simple(S, role):
            continue
        rs, a, nor, ho, ta, tnor = S.sets[role]
        fin = np.isfinite(a)
        pts = [rs.rays[:, :3]]
        for off in (-R.F3_EPS, R.F3_EPS):
            pts.append(R.ray_pos(rs.rays[fin, :3], rs.rays[fin, 3:], a[fin] + off))
        pts = np.concatenate(pts)
        want = oracle.obj_sides(S.flat, e, pts)
        q = np.concatenate([pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1))], axis=1)
        for lds, prune in variants(h, S.root):
            for op in ("side_lane", "side_uni"):
                g = h.query_rays(op, e, q, lds=lds, prune=prune)[:, 0]
                bad = g != want
                assert not bad.any(), f"{op} lds={lds} prune={prune} on {role}: {int(bad.sum())} of {len(pts)} points, first {pts[np.flatnonzero(bad)[0]].tolist()}"
        if role in R.TORUS_ROLES:
            assert len(set(want[:len(rs)][rs.cls == "torus_axis"])) == 2, role   # axis and centre circle: both answers occur


# ---- 3. the rough simple compound ---------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{}, {"ACN_NO_SC_CULL": 1}, {"ACN_NO_SC_REVERSED": 1}], ids=["culled", "no_cull", "one_order"])
def test_rough_compound(env, S, oracle):
    """simple_compound_hit on rough_compound (64 spheres, every second one rough through the table's ACN_SC_ROUGH flag, each
    rough sphere bit-tied with a smooth twin): distance, normal and hit object of the oracle's compound_s_ray_hit; the any-hit
    column against a <= limit"""
    e = S.elems["rough_compound"]
    rs, a, nor, ho, ta, tnor = S.sets["rough_compound"]
    fin = np.isfinite(a)
    h = upload(S.flat, **env)
    try:
        info = h.query_rays("elements", S.root, n=len(S.elems))
        assert int(info[list(S.elems.values()).index(e), 1]) & 4, "rough_compound is no simple compound"
        rng = np.random.default_rng(29)
        lim = np.where(fin, a + rng.choice([0.0, R.F3_EPS, -R.F3_EPS, 1.0], len(a)), 1.0)
        for lds in (True, False):
            g = h.query_rays("sc_hit", e, rs.rays, limits=lim, lds=lds)
            bad = (bits(g[:, 0]) != bits(a)) | (fin & ((g[:, 4] != ho) | (bits(g[:, 1:4]) != bits(nor)).any(axis=1)))
            assert not bad.any(), report_mismatch(f"simple_compound_hit {env} lds={lds}", "rough_compound", rs, bad)
            bad = (g[:, 5] != 0) != (a <= lim)
            assert not bad.any(), report_mismatch(f"simple_compound_hit any-hit form {env} lds={lds}", "rough_compound", rs, bad)
    finally:
        h.close()
    r = np.array([S.flat.node(int(k)).surface_roughness if k >= 0 else 0.0 for k in ho])
    ties = rs.cls == "ties"
    print(f"rough_compound {env}: hits on a rough sphere {int((fin & (r > 0)).sum())}, on a smooth one {int((fin & (r == 0)).sum())}, "
          f"of the tie class {int((fin & ties).sum())}")
    assert (fin & (r > 0)).sum() >= 100 and (fin & (r == 0)).sum() >= 100 and (fin & ties).sum() >= 50


# ---- 4. scene level -----------------------------------------------------------------------------------------------

def test_trans_and_occlusion(S, handles, oracle):
    """root_trans_hit (full, fast, resumed) and root_occluded (all three answers) on the matter root, as
    test_gpu_queries.test_trans_and_occlusion asserts them"""
    rs = R.rough_distance_scene_rays(np.random.default_rng(3), oracle, S.flat)
    a, _, _ = oracle.compound_ray_hits(S.flat, S.root, rs.rays)
    special = {S.elems[r] for r in S.roles if S.rough_nodes(r) or R.tori_of(S.flat, S.elems[r]) or r.startswith("sdf")}
    counts, queries = check_trans_and_occlusion(S.flat, {k: handles[k] for k in ("default", "prune_min_1")}, rs, a, oracle, special)
    print("scene queries:", dict(counts), "rays", len(rs), "occlusion queries", queries)
    for hname in ("default", "prune_min_1"):
        assert counts[("trans_hard", hname)] >= 20 and counts[("trans_hard_special", hname)] >= 5, dict(counts)
        assert counts[("occluded_hard", hname)] > 0


# ---- 5. prune -----------------------------------------------------------------------------------------------------

def test_prune(S, handles):
    """distance objects are never pruned: 0, 0, 0 on the distance roles; on the pairs and trees that hold a torus a skip never
    drops a finite oracle hit"""
    skips = Counter()
    for hname in ("default", "prune_min_1"):
        h = handles[hname]
        for role in R.DISTANCE_ROLES + ("rough_torus", "torus_and_ball", "torus_deep", "torus_minus_half", "torus_hole"):
            rs, a, *_ = S.sets[role]
            for lds, prune in variants(h, S.root):
                g = h.query_rays("prune", S.elems[role], rs.rays, limits=np.full(len(rs), np.inf), lds=lds, prune=prune)
                if S.flat.node(S.elems[role]).type == R.ACN_DISTANCE:
                    assert not g[:, :3].any(), f"prune ({hname}) on {role}: a distance object was pruned"
                else:
                    skip = (g[:, 0] != 0) | (g[:, 2] != 0)
                    bad = skip & np.isfinite(a)
                    assert not bad.any(), report_mismatch(f"prune ({hname}, lds={lds}, prune={prune}) skipped a hit", role, rs, bad)
                    skips[(hname, role)] += int(skip.sum())
    print("prune skips:", dict(skips))
    assert skips[("default", "torus_and_ball")] + skips[("prune_min_1", "torus_and_ball")] >= 20


# ---- 6. wave independence -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("role", ["torus", "torus_short", "rough_tree"])
def test_wave_independence(role, S, handles, oracle):
    """the march's trip count differs per lane: 256 rays, each alone in its wave (lane k % 64, the other 63 lanes a far miss),
    and the same rays in one shuffled batch -- the same bits, and the oracle's"""
    h = handles["prune_min_1"]
    e = S.elems[role]
    rs, a, nor, *_ = S.sets[role]
    rng = np.random.default_rng(37)
    hit, miss = np.flatnonzero(np.isfinite(a)), np.flatnonzero(~np.isfinite(a))
    pick = np.concatenate([rng.choice(hit, min(160, len(hit)), replace=False), rng.choice(miss, 256 - min(160, len(hit)), replace=False)])
    c, rad = R.node_ball(S.flat, e)
    cand = R.far(np.random.default_rng(1), c + np.array([0, 0, 50.0]), 1.0, 64).rays   # aimed 50 units past the element
    fa, _ = oracle.obj_ray_hits(S.flat, e, cand)
    filler = cand[np.flatnonzero(~np.isfinite(fa))[0]]
    alone = np.tile(filler, (256 * 64, 1))
    slot = np.arange(256) * 64 + np.arange(256) % 64
    alone[slot] = rs.rays[pick]
    order = rng.permutation(256)
    for op in ("hit_lane", "hit_uni", "element_hit"):
        g1 = h.query_rays(op, e, alone)
        assert not np.isfinite(np.delete(g1[:, 0], slot)).any()
        g1 = g1[slot]
        g2 = np.empty_like(g1)
        g2[order] = h.query_rays(op, e, rs.rays[pick][order])
        sub = R.RaySet(rs.rays[pick], rs.cls[pick])
        bad = (bits(g1[:, :5]) != bits(g2[:, :5])).any(axis=1)
        assert not bad.any(), report_mismatch(f"{op} depends on which rays share the wave", role, sub, bad)
        bad = (bits(g1[:, 0]) != bits(a[pick])) | (np.isfinite(a[pick]) & (bits(g1[:, 1:4]) != bits(nor[pick])).any(axis=1))
        assert not bad.any(), report_mismatch(f"{op}, one ray per wave", role, sub, bad)


# ---- 7. the twin on the device, and the counts --------------------------------------------------------------------

def test_twin_and_model_on_device(S, handles, oracle, detmath_cpu):
    """the device's own outputs on both sides: the rough handle's distances have the bits of the twin handle's, and its
    normals equal rough_model.roughen of the twin handle's normals, node by node (rough_model.check_rough_steps with
    hit_lane and side_lane of the two handles); on rough_compound through sc_hit"""
    hr, ht = handles["default"], handles["twin"]

    def dev(h):
        def f(node, rays):
            g = h.query_rays("hit_lane", node, rays)
            return g[:, 0], g[:, 1:4]
        return f

    def sides(node, pts):
        return hr.query_rays("side_lane", node, np.concatenate([pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1))], axis=1))[:, 0].astype(np.int64)
    total = Counter()
    differ = {}
    a_of = {}
    for role, e in S.elems.items():
        rs = S.sets[role][0]
        op = "hit_lane" if simple(S, role) else "sc_hit"
        g, t = hr.query_rays(op, e, rs.rays), ht.query_rays(op, e, rs.rays)
        a_of[role] = g[:, 0]
        assert (bits(g[:, 0]) == bits(t[:, 0])).all(), f"{role}: the rough handle's distances differ from the twin handle's"
        fin = np.isfinite(g[:, 0])
        differ[role] = int((fin & (bits(g[:, 1:4]) != bits(t[:, 1:4])).any(axis=1)).sum())
        if simple(S, role):
            stats = {}
            bad = M.check_rough_steps(S.flat, S.twin, e, rs.rays, dev(hr), dev(ht), sides, oracle, detmath_cpu, stats)
            assert bad == 0, f"{role}: {bad} normals of the device differ from the model; first {stats.get('first_bad')}"
            total.update({k: v for k, v in stats.items() if k != "first_bad"})
        else:
            assert (g[fin, 4] == t[fin, 4]).all()
            r = np.array([S.flat.node(int(k)).surface_roughness if k >= 0 else 0.0 for k in g[:, 4]])
            want = t[:, 1:4].copy()
            for v in set(r[fin & (r > 0)]):
                m = fin & (r == v)
                want[m] = M.roughen(t[m, 1:4], R.ray_pos(rs.rays[m, :3], rs.rays[m, 3:], g[m, 0]), float(v), oracle, detmath_cpu)
            assert (bits(want[fin]) == bits(g[fin, 1:4])).all(), f"{role}: normals of the device differ from the model"
    print("model on the device, all roles:", dict(total))
    for k in ("rough_leaf", "rough_pair", "rough_neg", "rough_scale"):
        assert total[k] >= 100, (k, dict(total))
    # not vacuous, on the device's answers
    S.check_counts(S.counts(a_of))
    for role in S.roles:
        print("normals that differ from the twin's:", role, differ[role])
        if S.rough_nodes(role):
            assert differ[role] >= 100, (role, differ[role])
        else:
            assert differ[role] == 0, (role, differ[role])

"""What tests/test_gpu_queries.py and tests/test_gpu_rough_distance.py share: handles uploaded under an upload-time environment,
the bit comparison and its failure report, and the scene-level comparison of root_trans_hit / root_occluded with the oracle."""
import os
from collections import Counter

import numpy as np

import actinon_amd as A
import ray_sets as R

# (lds, prune).  The query scene is too big to be staged in LDS (the upload step stages at most ~4 KB of nodes, and only for
# roots with generic nested compounds): its handles read nodes from global memory and the queries run the two scene views;
# test_lds_staged_nodes runs a scene that is staged, in both placements
VARIANTS = [(False, True), (False, False)]
MACHINE_TYPES = (R.ACN_PAIR_INSIDE, R.ACN_PAIR_OUTSIDE, R.ACN_NEG, R.ACN_SCALE)


def upload(flat, **env):
    """a handle of `flat` uploaded with the given upload-time environment (ACN_PRUNE_MIN, ACN_NO_SC_*)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return A.Handle(flat)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def report_mismatch(what, role, rs, bad):
    cls = Counter(rs.cls[bad])
    k = int(np.flatnonzero(bad)[0])
    return f"{what} on {role}: {int(bad.sum())} of {len(rs)} rays differ, by class {dict(cls)}; first: ray {rs.rays[k].tolist()}"


def check_trans_and_occlusion(flat, handles, rs, a, oracle, special=()):
    """TRANS (root_trans_hit, and root_trans_hit_fast with the hard redo) equals the oracle's compound_s_ray_trans_hit;
    root_occluded and root_occluded_fast equal compound_s_ray_hit( matter ) <= limit (a: the oracle's distances of rs on the
    matter root), and the fast form answers 2 (hard) only where a machine element of the root was not ruled out.  Returns
    ( counts of hard answers per handle, number of occlusion queries ); special: root elements whose hits among the hard trans
    answers are counted too."""
    root = flat.c.matter_root
    ta, tn, tex, ten = oracle.trans_hits(flat, root, rs.rays)
    els = flat.elems_of(root)
    rng = np.random.default_rng(9)
    idx, lim = R.occlusion_limits(a, rng)
    want = a[idx] <= lim
    counts = Counter()
    for hname, h in handles.items():
        info = h.query_rays("elements", root, n=len(els))
        machine = [int(info[k, 0]) for k in range(len(els)) if not (int(info[k, 1]) & 7)]
        for lds, prune in VARIANTS:
            g = h.query_rays("trans", root, rs.rays, lds=lds, prune=prune)
            for off, form in ((0, "root_trans_hit"), (6, "root_trans_hit_fast")):
                bad = bits(g[:, off]) != bits(ta)
                fin = np.isfinite(ta)
                bad |= fin & (bits(g[:, off + 1:off + 4]) != bits(tn)).any(axis=1)
                bad |= fin & ((g[:, off + 4] != tex) | (g[:, off + 5] != ten))
                assert not bad.any(), report_mismatch(f"{form} ({hname}, lds={lds}, prune={prune})", "matter root", rs, bad)
            counts[("trans_hard", hname)] += int(g[:, 12].sum())
            if special:
                counts[("trans_hard_special", hname)] += int(((g[:, 12] != 0) & np.isfinite(ta) & np.isin(tex, list(special))).sum())
            o = h.query_rays("occluded", root, rs.rays[idx], limits=lim, lds=lds, prune=prune)
            sub = R.RaySet(rs.rays[idx], rs.cls[idx])
            bad = (o[:, 0] != 0) != want
            assert not bad.any(), report_mismatch(f"root_occluded ({hname}, lds={lds}, prune={prune})", "matter root", sub, bad)
            f = o[:, 1]
            bad = ((f == 0) & want) | ((f == 1) & ~want)
            assert not bad.any(), report_mismatch(f"root_occluded_fast ({hname}, lds={lds}, prune={prune})", "matter root", sub, bad)
            hard = np.flatnonzero(f == 2)
            counts[("occluded_hard", hname)] += len(hard)
            if len(hard) and prune:
                # a hard answer needs a machine element that was not ruled out (envelope hit, not pruned)
                live = np.zeros(len(hard), bool)
                for m in machine:
                    t = flat.node(m).type
                    if t in MACHINE_TYPES:
                        p = h.query_rays("prune", m, sub.rays[hard], limits=lim[hard], lds=lds, prune=prune)
                        live |= (p[:, 0] == 0) & (p[:, 1] == 0)
                    elif t in (R.ACN_COMPOUND, R.ACN_DISTANCE):
                        # what root_occluded_fast asks of them: no envelope, or the ray enters it (env_ray_hits)
                        live |= env_enters(flat.node(m), sub.rays[hard])
                    else:
                        raise AssertionError(f"element {m} of type {t}: no rule for a hard answer")
                assert live.all(), f"root_occluded_fast ({hname}) answered hard on {int((~live).sum())} rays with every machine element ruled out"
    return counts, len(idx)

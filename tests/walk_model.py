"""The specular walk of one path level (acn_k_walk.h: k_walk) as a worklist over the oracle.  No arithmetic is restated here: a ray's
hit is Oracle.trans_hit, what the hit produces is Oracle.shade_point (scene_lum for one hit, recorded while it runs) turned into
records by shade_model.split_expected, and the only term the walk adds itself -- the background of a miss -- is
to_fixed( T * ( background * intensity ) ), the order of v_mld( T, v_mlf( bg, intensity ) ).

The arrangement of the walk (passes, private stacks, fetch batch, grid) decides where a ray is traced, never what it produces, so one
expectation stands for every arrangement: the rays of every generation, all tasks and probes, and accum as the exact int64 sum of the
per-ray fixed-point terms (an integer sum: the same in any order)."""
import numpy as np

import shade_model as M

INVALID = M.INVALID


class Walk:
    """gens[ g ]: the live rays of generation g (numpy "ray" records; gens[ 0 ]: the live input); tasks, probes: lists of records;
    accum [ n, 3 ] int64; the totals as attributes"""

    def __init__(self, n):
        self.gens, self.tasks, self.probes = [], [], []
        self.accum = np.zeros((n, 3), dtype=np.int64)
        self.misses = self.emissions = self.clamped = 0
        self.terms = np.zeros(n, dtype=np.int64)          # fixed-point terms per pixel (roundings to the 2^-40 grid)
        self.subtree = np.zeros(n, dtype=np.int64)        # rays per pixel, the input ray included

    rays = property(lambda self: sum(len(g) for g in self.gens))
    generations = property(lambda self: len(self.gens))

    def totals(self):
        return {"rays": self.rays, "generations": self.generations, "tasks": len(self.tasks), "probes": len(self.probes),
                "emissions": self.emissions, "misses": self.misses, "largest_subtree": int(self.subtree.max()) if len(self.subtree) else 0}

    def rays_at_depth(self, depth):
        return sum(int((g["depth"] == depth).sum()) for g in self.gens)


def _trace(oracle, flat, r, records, emit_terms):
    """one ray: (children, probes, task or None, term int64 [3], is a term, clamps, miss, emission)"""
    prm = flat.params
    a, nor, ex, en = oracle.trans_hit(flat, r["p"], r["d"])
    if not a < np.inf:
        v = r["T"] * (np.array(list(prm.background_color)) * r["intensity"])
        return [], [], None, M.to_fixed(v), True, bool((np.abs(v) > M.FIX_CLAMP).any()), True, False
    hit = np.zeros((), dtype=records["hit"])
    hit["p"], hit["d"], hit["offs"], hit["exit_nor"], hit["T"], hit["intensity"] = r["p"], r["d"], a, nor, r["T"], r["intensity"]
    hit["exit_obj"], hit["enter_obj"], hit["depth"], hit["pixel"] = ex, en, r["depth"], r["pixel"]
    rows = oracle.shade_point(flat, M.tap_input(hit))[0]
    children, probes, task, term = M.split_expected(rows, hit, prm, records, emit_terms=emit_terms)
    em = M.rows_of(rows, "emission")
    clamp = bool(len(em)) and bool((np.abs(r["T"] * em[0, 1:4]) > M.FIX_CLAMP).any())
    return children, probes, task, term, len(em) > 0, clamp, False, len(em) > 0


def walk(oracle, flat, rays, records, n=None, emit_terms=True, memo=None):
    """The walk from `rays` ("ray" records; dead slots, pixel INVALID, are skipped): every generation until none is left.  n: pixels of
    accum (default: the number of input records).  `rays` may be the rays a device run left over: the model then continues from them.
    emit_terms False: no probes, and the walk's own terms are dropped (k_walk: if( live && emit_terms ) pixel_add).  memo: a dict that
    keeps what a ray produced by the bytes of its record, so that a continuation does not ask the oracle again."""
    rays = np.asarray(rays, dtype=records["ray"])
    w = Walk(len(rays) if n is None else n)
    gen = [r for r in rays if r["pixel"] != INVALID]
    while gen:
        w.gens.append(np.array(gen, dtype=records["ray"]))
        nxt = []
        for r in gen:
            key = (np.asarray(r).tobytes(), bool(emit_terms))
            res = memo.get(key) if memo is not None else None
            if res is None:
                res = _trace(oracle, flat, r, records, emit_terms)
                if memo is not None:
                    memo[key] = res
            children, probes, task, term, is_term, clamp, miss, emission = res
            px = int(r["pixel"])
            w.subtree[px] += 1
            w.misses += int(miss)
            w.emissions += int(emission)
            nxt += children
            w.probes += probes
            if task is not None:
                w.tasks.append(task)
            if emit_terms:
                w.accum[px] += term
                w.terms[px] += int(is_term)
                w.clamped += int(clamp)
        gen = nxt
    return w


def ledger(oracle, flat, rays, records):
    """What k_walk< COUNT > books for the walk from `rays`, all generations (shade_model.ledger_hit with the device's differences), and
    the rays [m, 6] it traces: (ledger, traced).  One scene_s_trans_hit per ray -- two compound_s_ray_trans_hit calls -- and shade_hit
    for every hit; a dead child stands for two more (DEVICE_DEAD_CHILD)."""
    prm = flat.params
    gen = [r for r in np.asarray(rays, dtype=records["ray"]) if r["pixel"] != INVALID]
    parts, traced, trans = [], [], 0
    while gen:
        nxt = []
        for r in gen:
            traced.append(np.concatenate([r["p"], r["d"]]))
            trans += 2
            a, nor, ex, en = oracle.trans_hit(flat, r["p"], r["d"])
            if not a < np.inf:
                continue
            hit = np.zeros((), dtype=records["hit"])
            hit["p"], hit["d"], hit["offs"], hit["exit_nor"], hit["T"], hit["intensity"] = r["p"], r["d"], a, nor, r["T"], r["intensity"]
            hit["exit_obj"], hit["enter_obj"], hit["depth"], hit["pixel"] = ex, en, r["depth"], r["pixel"]
            rows = oracle.shade_point(flat, M.tap_input(hit))[0]
            parts.append(M.ledger_hit(rows, a, prm, device=True))
            nxt += M.split_expected(rows, hit, prm, records)[0]
        gen = nxt
    out = M.add_ledgers(parts)
    out["trans_ray"] += trans
    return out, np.array(traced).reshape(-1, 6)

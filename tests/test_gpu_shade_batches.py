"""The batched set-up of k_shade< 16 > (acn_k_shade.h, BATCHED): a wave takes 16 tasks at a time, sets them up one task per lane, light
by light, and runs their sample loops four tasks at a time against the frames the set-up left in LDS.  What a batch can get wrong and a
step of four tasks could not: which frame a group reads, what a dead index entry leaves behind, the values a task carries from light
to light and into the path loop (rv, lum) now that they live in the frame, neighbours in a batch that differ in every branch of the
set-up.  On hand-made queues through the stage seam, as tests/test_gpu_shade_loops.py does, and against its three references:

  class 4      the three output queues, as sorted byte strings, are those of the same tasks on 4 lanes per task: that kernel keeps the
               plain step of four tasks, set up by every lane of a group.  Both forms expand one definition of the set-up, so
               what this comparison guards is the batching itself: the frames, the sub-steps, what a task carries in LDS
  the tap      every record is a sample of the oracle's scene_lum at that point (check_records)
  the sums     accum equals exact_accum for 16 lanes per task, bit for bit

The seam chooses the grid itself, one workgroup per four index entries and 64 at most: up to four entries run on one workgroup, the
larger counts on several, where each batch of 16 goes to whichever wave draws it.  What one wave carries from a batch into its next is
the last case's: a list with more live batches than the grid has waves."""
import types

import numpy as np
import pytest

import actinon_amd as A
from actinon_amd._lib import host
import ray_sets as R
import shade_model as M
import test_gpu_shade_loops as L

pytestmark = pytest.mark.gpu

REC = A.Handle.STAGE_RECORDS
DEAD = A.Handle.STAGE_INVALID
LIFT = L.LIFT
CARRIER_AT = (40.0, 40.0, 3.0)             # a small ball far from everything: the surface of the tasks with on_b = 0


class BatchQueue(L.Queue):
    """L.Queue with the surface of every point named: points are ( pos, n, depth, k ), k the position of the entered object in the
    matter root (0: the floor)"""

    def __init__(self, oracle, detmath, sc, points, seed=5):
        self.sc, self.flat = sc, sc.flatten()
        self.prm, self.oracle, self.detmath = self.flat.params, oracle, detmath
        self.h = A.Handle(self.flat, device=0)
        self.info = self.h.stage_info()
        self.st, self.expect = self, {}
        rng = np.random.default_rng(seed)
        matter = self.flat.elems_of(self.flat.c.matter_root)
        hits = []
        for pos, n, depth, k in points:
            d = (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0)
            hits.append(R._sample_point(REC["hit"], self.prm, matter[k], pos, (0, 0, 1), d, n, depth, rng.uniform(0.3, 1.0, 3)))
        self.hits = np.array(hits, dtype=REC["hit"])
        self.hits["pixel"] = np.arange(len(hits))
        self.rows = [oracle.shade_point(self.flat, M.tap_input(r))[0] for r in self.hits]
        self.tasks = np.array([M.task_of(rw, r, REC) for r, rw in zip(self.hits, self.rows)], dtype=REC["task"])
        self.counts = [M.sample_counts(rw) for rw in self.rows]


def view(q, sel):
    """the tasks `sel` of q as a queue of their own, numbered from 0: what check_records and exact_accum read of a queue"""
    sel = list(sel)
    tasks = q.tasks[sel].copy()
    tasks["pixel"] = np.arange(len(sel))
    return types.SimpleNamespace(prm=q.prm, flat=q.flat, detmath=q.detmath, h=q.h, tasks=tasks, rows=[q.rows[i] for i in sel],
                                 counts=[q.counts[i] for i in sel])


def check(q, sel, index=None, cls=1, shard=(0, 1)):
    """the three references of the module's docstring for the tasks `sel`, reached through `index` (default: all, in order)"""
    v = view(q, sel)
    kw = dict(index=index, shard_rank=shard[0], shard_world=shard[1])
    got, ref = v.h.run_stage("shade", v.tasks, cls=cls, **kw), v.h.run_stage("shade", v.tasks, cls=2, **kw)
    assert got["flags"] == 0 and ref["flags"] == 0, (got["flags"], ref["flags"])
    for name in L.QUEUES:
        L.G.same_records(got[name], list(ref[name]), (name, len(sel)))
    tally = L.check_records(v, got, shard=shard)
    want = L.exact_accum(v, got, L.LANES[cls], shard=shard)
    assert np.array_equal(got["accum"], want), ("accum", np.nonzero((got["accum"] != want).any(axis=1))[0])
    return tally, got


def _carrier(sigma):
    o = host.acn_obj_sphere_s_create(0.05)
    host.acn_obj_set_material(o, b"diffuse")
    host.acn_obj_set_sigma(o, sigma)
    host.acn_obj_move(o, A.v3(*CARRIER_AT))
    return o


def scene(lights, samples):
    """L.build's floor, glass torus and sphere, and behind them the carrier ball (matter position 3)"""
    sc = L.build(lights, ["glass", (0.4, (2.0, 0.6, 2.2))], direct_samples=samples, path_samples=samples)
    o = _carrier(0.0)
    sc.push(o)
    host.acn_obj_discard(o)
    return sc


# 33 points of two lights: counts around the group's 16 lanes, with and without a path loop, every fourth on the carrier's surface
def _points33():
    rng = np.random.default_rng(11)
    counts = (9, 15, 16, 17, 40, 12, 33, 10)
    return tuple(((rng.uniform(-2.0, 3.0), rng.uniform(-3.0, 2.0), LIFT), counts[k % 8], (12, 22, 10)[k % 3], 3 if k % 4 == 3 else 0) for k in range(33))


@pytest.fixture(scope="module")
def queue33(oracle, detmath_cpu):
    q = BatchQueue(oracle, detmath_cpu, scene(("sphere", "plane"), 40), _points33())
    yield q
    q.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 33])
def test_task_counts(queue33, n):
    """part of a sub-step, a sub-step, part of a batch, a batch, a batch and one task, two batches and one task; two lights: the
    second light's loop starts from the rv the first one's left in the frame, and adds to its lum"""
    q = queue33
    assert q.info["lights"] == 2
    tally, _ = check(q, range(n))
    assert tally["inline"] > 0
    if n >= 15:
        assert tally["background"] > 0, tally


DEAD_LISTS = {
    "first":     [DEAD] + list(range(20)),
    "middle":    list(range(6)) + [DEAD] + list(range(6, 20)),
    "last":      list(range(15)) + [DEAD] + list(range(15, 20)),
    "sub_step":  list(range(4)) + [DEAD] * 4 + list(range(4, 20)),
    "batch":     [DEAD] * 16 + list(range(20)),
    "scattered": [DEAD, 0, DEAD, DEAD, 1, 2, 3, DEAD, 4, 5, 6, 7, 8, 9, 10, DEAD, DEAD, 11, 12, 13, DEAD, 14, 15, 16, 17, 18, 19, DEAD],
}


@pytest.mark.parametrize("where", list(DEAD_LISTS))
def test_dead_index_entries(queue33, where):
    """a dead entry leaves a dead frame: no group runs it, its lane sets nothing up and adds nothing"""
    index = DEAD_LISTS[where]
    assert sorted(i for i in index if i != DEAD) == list(range(20))
    check(queue33, range(20), index=index)


def test_sharded(queue33):
    """rank 1 of 3: the share of every loop starts at the jump from the frame's rv"""
    tally, _ = check(queue33, range(17), shard=(1, 3))
    assert tally["inline"] > 0


@pytest.mark.parametrize("n", [1, 2, 17])
def test_class_64(queue33, n):
    """the widest class keeps its step of one task"""
    check(queue33, range(n), cls=0)


# ---------------------------------------------------------------------------------------------------------------------
# one wave, several batches.  The seam's grid is at most 64 workgroups, 256 waves, and a list of a few thousand entries is handed out
# in batches of 16 (balanced_batch at its floor).  Here EVERY batch holds a live task, and there are more batches than waves: some
# waves go round the batched loop twice and more (in fact nearly all: a wave reserves its next batch while it works the first), and
# whenever one does, a live batch follows a live one in the frames of that wave.

CARRY_BATCHES = 321                            # > 256 waves; the last one is short: got = 5


def _carry_layout():
    """the index list, batch by batch: 16 live entries in every 64th batch, 3 in every 8th, 1 elsewhere, from a lane that moves
    with the batch; the rest dead.  The last batch has 5 entries, 2 of them live."""
    index, n = [], 0
    for b in range(CARRY_BATCHES):
        size = 16 if b < CARRY_BATCHES - 1 else 5
        live = 2 if size == 5 else 16 if b % 64 == 0 else 3 if b % 8 == 4 else 1
        first = (b * 5) % size
        at = {(first + k) % size for k in range(live)}
        for k in range(size):
            if k in at:
                index.append(n)
                n += 1
            else:
                index.append(DEAD)
    return index, n


@pytest.fixture(scope="module")
def carry_queue(oracle, detmath_cpu):
    _, n = _carry_layout()
    rng = np.random.default_rng(31)
    counts = (9, 10, 12, 16, 17, 9, 11, 9)
    points = tuple(((rng.uniform(-2.0, 3.0), rng.uniform(-3.0, 2.0), LIFT), counts[k % 8], (12, 10, 22)[k % 3], 3 if k % 5 == 4 else 0) for k in range(n))
    q = BatchQueue(oracle, detmath_cpu, scene(("sphere",), 20), points)
    yield q
    q.close()


def test_waves_take_several_batches(carry_queue):
    """what a wave carries from one batch into the next: the frames and task slots of the batch before (a dead entry now where a
    live one was, a short last batch over the frames of a whole one), the fetch range going on in units of 16, the wave's queue
    reservations.  Same three references."""
    q = carry_queue
    index, n = _carry_layout()
    assert len(index) == 16 * (CARRY_BATCHES - 1) + 5 and len(index) > 64 * 4 * 16 and n == len(q.tasks)
    tally, got = check(q, range(n), index=index)
    assert tally["inline"] > 0 and tally["background"] > 0, tally
    print("carry:", n, "tasks in", CARRY_BATCHES, "batches", tally)


def test_mixed_batch(oracle, detmath_cpu):
    """16 tasks, one batch: neighbours differ in on_b, in the sample count (9 and 255), in having a path loop, in the cone cull (a point
    inside the sphere light culls nothing: cos_theta <= 1e-6), under three lights of two kinds"""
    inside = L.INSIDE_POINTS[0][0]
    rng = np.random.default_rng(23)
    rnd = lambda: (rng.uniform(-2.0, 3.0), rng.uniform(-3.0, 2.0), LIFT)     # noqa: E731
    points = (((0.5, -0.5, LIFT), 9, 12, 0), (rnd(), 255, 22, 3), (inside, 17, 12, 0), (rnd(), 17, 10, 0),
              (rnd(), 9, 10, 3), ((0.5, -0.5, LIFT), 255, 12, 0), (rnd(), 9, 22, 3), (inside, 40, 10, 3),
              (rnd(), 16, 12, 0), (rnd(), 255, 10, 3), (rnd(), 9, 12, 0), (rnd(), 33, 22, 3),
              (rnd(), 15, 10, 0), ((6.0, -6.0, LIFT), 40, 12, 3), (rnd(), 9, 12, 0), (rnd(), 255, 12, 3))
    q = BatchQueue(oracle, detmath_cpu, scene(("plane", "sphere_env", "sphere"), 256), points)
    try:
        assert q.info["lights"] == 3
        on_b = q.tasks["on_b"]
        assert [bool(b > 0) for b in on_b] == [p[3] == 0 for p in points]
        assert [c[0] for c in q.counts] == [p[1] for p in points]
        assert [c[1] for c in q.counts] == [p[1] if p[2] > 10 else 0 for p in points]
        masks = L.cull_masks(q, light=2)                       # the plain sphere light
        assert masks[2] == 0 and masks[7] == 0 and masks[1] != 0 and masks[13] != 0, [bin(m) for m in masks]
        tally, got = check(q, range(16))
        for k in ("hard_shadow", "inline", "background"):
            assert tally[k] > 0, tally
        print("mixed batch:", tally)
    finally:
        q.close()

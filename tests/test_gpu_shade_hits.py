"""k_shade_hits at the edges of its steps of 64 records: the production kernel on queues the test wrote, through acn_run_stage, against
the oracle's tap and tests/shade_model.py as tests/test_gpu_stages.py does -- at the input sizes where the last step is partial, with
dead records at the places a step can have them, on an input large enough that a wave takes several batches and its appends cross
reservations inside a step (the wave's probe count, added once when the wave ends, is then the sum over many steps), and through a
frame whose chunks overflow their queues, which runs the cap guards of the appends."""
import numpy as np
import pytest

import actinon_amd as A
import ray_sets as R
import shade_model as M
from test_gpu_stages import Stage, same_records

pytestmark = pytest.mark.gpu

REC = A.Handle.STAGE_RECORDS
QC = A.Handle.QC
INVALID = A.Handle.STAGE_INVALID
ACN_FLAG_CLAMPED = 8
KINDS = ("two_children", "probes", "diffuse_only", "emission")


@pytest.fixture(scope="module")
def stage(oracle):
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"
    s = Stage(oracle, False)
    yield s
    s.h.close()


class Base:
    """The live records of the split test (ray_sets.stage_split_hits on scene A) with what the model expects of each, computed once:
    every test below repeats these records under other pixels."""

    def __init__(self, st):
        recs = R.stage_split_hits(st.oracle, st.flat, st.node, REC["hit"])
        self.recs = recs[recs["pixel"] != INVALID]
        arr = lambda l, k: np.array(l, dtype=REC[k]) if len(l) else np.zeros(0, dtype=REC[k])   # noqa: E731
        self.rays, self.probes, self.tasks, self.acc = [], [], [], []
        for r, rw in zip(self.recs, st.tap(self.recs)):
            rays, probes, task, acc = M.split_expected(rw, r, st.prm, REC)
            self.rays.append(arr(rays, "ray")); self.probes.append(arr(probes, "hard_shadow"))
            self.tasks.append(arr([task] if task is not None else [], "task")); self.acc.append(acc)
        self.acc = np.array(self.acc)
        n_rays, n_probes, n_tasks = (np.array([len(x) for x in q]) for q in (self.rays, self.probes, self.tasks))
        emits = (self.acc != 0).any(axis=1)
        self.kind = {"two_children": np.nonzero(n_rays >= 2)[0], "probes": np.nonzero(n_probes > 0)[0],
                     "diffuse_only": np.nonzero((n_tasks == 1) & (n_rays == 0) & (n_probes == 0))[0], "emission": np.nonzero(emits)[0]}
        for k in KINDS:
            assert len(self.kind[k]) >= 3, (k, len(self.kind[k]))
        # the four kinds in turn, then everything else: the first records of any input hold every kind
        m = min(len(self.kind[k]) for k in KINDS)
        first = np.stack([self.kind[k][:m] for k in KINDS], axis=1).reshape(-1)
        self.order = np.concatenate([first, np.setdiff1d(np.arange(len(self.recs)), first)])

    def records(self, src, dead):
        """hit records src (indices into the base) with pixel = own index, dead ones INVALID, and what the kernel is to make of them"""
        n = len(src)
        recs = self.recs[src].copy()
        recs["pixel"] = np.arange(n)
        recs["pixel"][dead] = INVALID
        live = np.nonzero(~dead)[0]
        want = {}
        for name, per_base, kind in (("rays", self.rays, "ray"), ("probes", self.probes, "hard_shadow"), ("tasks", self.tasks, "task")):
            parts = [per_base[b] for b in src[live]]
            q = np.concatenate(parts) if parts else np.zeros(0, dtype=REC[kind])
            q["pixel"] = np.repeat(live, [len(p) for p in parts]) if parts else []
            want[name] = q
        want["accum"] = np.zeros((n, 3), dtype=np.int64)
        want["accum"][live] = self.acc[src[live]]
        return recs, want


@pytest.fixture(scope="module")
def base(stage):
    return Base(stage)


def classes_of(st, tasks):
    nd = np.maximum((st.prm.direct_samples * tasks["diffuse_intensity"]).astype(np.int64), 1)
    npth = np.where(tasks["depth"] > 10, np.maximum((st.prm.path_samples * tasks["diffuse_intensity"]).astype(np.int64), 1), 0)
    return np.array([M.size_class(int(v), st.info["class0_min"]) for v in np.maximum(nd, npth)], dtype=np.int64)


def run_and_compare(st, base, src, dead):
    """the whole of what k_shade_hits wrote for the records, as sets and bit for bit; returns the output"""
    recs, want = base.records(np.asarray(src), np.asarray(dead, dtype=bool))
    out = st.h.run_stage("shade_hits", recs)
    same_records(out["rays"], list(want["rays"]), "rays")
    same_records(out["hard_shadow"], list(want["probes"]), "probes")
    assert (out["hard_shadow"]["pad"] == 1).all()
    listed = np.concatenate(out["idx"])
    assert len(np.unique(listed)) == len(listed) == len(want["tasks"])
    same_records(out["tasks"][listed.astype(np.int64)], list(want["tasks"]), "tasks")
    for k in range(4):
        assert (classes_of(st, out["tasks"][out["idx"][k].astype(np.int64)]) == k).all(), k
    assert [len(l) for l in out["idx"]] == list(np.bincount(classes_of(st, want["tasks"]), minlength=4))
    c = out["counts"]
    assert c[QC["s_probes"]] == len(want["probes"]) and c[QC["tasks"]] - c[QC["dead_t"]] == len(want["tasks"])
    assert c[QC["gen0"]] - c[QC["dead_r"]] == len(want["rays"])
    assert out["flags"] & ~ACN_FLAG_CLAMPED == 0, out["flags"]
    assert bool(out["flags"] & ACN_FLAG_CLAMPED) == bool((np.abs(want["accum"]) == 16384 << 40).any())
    assert np.array_equal(out["accum"], want["accum"])
    # dead slots: at most the unused end of ONE reservation per wave and queue (chunk_close; the plan's slack is exactly that)
    slack = out["caps"].grid * 4 * out["caps"].chunk
    marks = {"tasks": (c[QC["dead_t"]], c[QC["tasks"]] - len(want["tasks"])), "rays": (c[QC["dead_r"]], c[QC["gen0"]] - len(want["rays"])),
             "probes": (None, c[QC["hard_shadow"]] - len(want["probes"]))}
    for k in range(4):
        marks[f"class{k}"] = (None, c[QC["class0"] + k] - len(out["idx"][k]))
    for name, (word, unused) in marks.items():
        assert 0 <= unused <= slack and (word is None or word == unused), (name, word, unused, slack)
    return out, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129])
def test_partial_steps(stage, base, n):
    """a last step of 1, 63 and 64 records, alone and behind one or two whole ones"""
    out, want = run_and_compare(stage, base, base.order[:n], np.zeros(n, dtype=bool))
    assert len(want["rays"]) + len(want["probes"]) + len(want["tasks"]) > 0 and (n < 4 or (want["accum"] != 0).any())


def test_dead_records(stage, base):
    """four steps: the first record dead, the last record dead, all dead, every other record dead; then the same before a partial step"""
    dead = np.zeros(256, dtype=bool)
    dead[0] = dead[127] = True
    dead[128:192] = True
    dead[192:256:2] = True
    out, want = run_and_compare(stage, base, base.order[:256], dead)
    assert len(want["tasks"]) > 20 and len(want["rays"]) > 40 and len(want["probes"]) > 20   # every queue is appended to
    run_and_compare(stage, base, base.order[:256 + 37], np.concatenate([dead, np.arange(37) % 2 == 1]))


def test_fifty_thousand_records(stage, base):
    """50 000 records on the seam's 64 workgroups: a wave takes about three batches, and its appends cross the 64-slot reservations
    inside a step.  Emission hits, diffuse-only hits, glass hits with two children and dark children, shuffled, a twentieth dead."""
    n = 50000
    rng = np.random.default_rng(50)
    src = rng.permutation(np.resize(base.order, n))
    dead = rng.random(n) < 0.05
    out, want = run_and_compare(stage, base, src, dead)
    live = src[~dead]
    for k in KINDS:
        assert np.isin(live, base.kind[k]).sum() > 1000, k
    assert out["caps"].grid == 64 and out["caps"].chunk == 64
    print(f"{n} records -> {len(want['rays'])} rays, {len(want['probes'])} probes, {len(want['tasks'])} tasks; dead slots: "
          f"tasks {out['counts'][QC['dead_t']]}, rays {out['counts'][QC['dead_r']]} of at most {64 * 4 * 64} each")
    assert len(want["rays"]) > n // 4 and len(want["probes"]) > n // 20 and len(want["tasks"]) > n // 8


def test_frame_with_overflowing_queues(monkeypatch):
    """The smoke shape with a workspace at its floor and the whole frame as one chunk: chunks overflow and are redone, so the appends
    meet slots at and beyond their queues' caps.  The frame is the roomy render's to the bit."""
    sc = A.Scene.build("wine_glass", image_width=160, image_height=90, path_samples=16, direct_samples=50)
    flat = sc.flatten()
    pos = A.main_pass_positions(160, 90)
    for name in ("ACN_WORKSPACE_MB", "ACN_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ACN_LANES", "1")
    h = A.Handle(flat)
    ref, st_ref = h.render_positions(pos, linear=True), h.last_stages()
    h.close()
    assert st_ref["retries"] == 0 and ref.std() > 1e-3
    monkeypatch.setenv("ACN_WORKSPACE_MB", "48")
    monkeypatch.setenv("ACN_CHUNK", str(len(pos)))
    h = A.Handle(flat)
    got, st = h.render_positions(pos, linear=True), h.last_stages()
    h.close()
    print(f"retries {st['retries']:.0f}, chunks {st['chunks']:.0f}")
    assert st["retries"] > 0, st
    assert np.array_equal(got, ref)

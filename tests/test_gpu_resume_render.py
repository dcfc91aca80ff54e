"""Whole frames through the resumed hard-ray kernels (acn_k_hard.h: k_hard_shadow, k_hard_path): records of k_shade,
which carry a resume word, and the probes of k_walk, which carry none, meet in one queue and one loop.  Small frames of
the scenes whose matter roots differ most -- 3 elements with a leaf pair beside a deep CSG object (wine_glass), 63 elements
with machine elements beyond the positions a word can name (the lamps), a distance object (textured) -- against the CPU
oracle, at both widths of a shading task, and once more with the queues forced to overflow (run on the MI355X: -m gpu)."""
import os

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-9
SAMPLES = dict(path_samples=8, direct_samples=16)   # the scenes keep their own trace_depth
FRAMES = {
    "wine_glass": dict(image_width=96, image_height=54),
    "paraffin_lamp": dict(image_width=48, image_height=64),
    "hanging_lamp": dict(image_width=48, image_height=64),
    "textured": {},
}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def load(name):
    ov = dict(FRAMES[name], **SAMPLES)
    if name == "wine_glass":
        return A.Scene.build("wine_glass", **ov).flatten()
    if name == "textured":
        sc = S.build_textured()
        sc.set(**ov)
        return sc.flatten()
    return A.Flat.load(os.path.join(HERE, "golden", "scenes", name + ".npz"), **ov)


@pytest.fixture(scope="module", params=list(FRAMES))
def frame(request, oracle):
    """the scene, its sample positions and the oracle's frame: computed once, shared, never written to"""
    flat = load(request.param)
    assert int(flat.params.path_samples) == 8 and int(flat.params.direct_samples) == 16
    pos = S.positions(flat)
    cpu = oracle.render_positions(flat, pos, linear=True)
    cpu.setflags(write=False)
    return request.param, flat, pos, cpu


def eight_bit(flat, lin):
    return A.cps_from_cl(np.clip(lin, 0, None) ** flat.params.gamma)


@pytest.mark.parametrize("wide", [False, True], ids=["tasks_on_16_lanes", "tasks_on_64_lanes"])
def test_frame_matches_oracle(frame, wide, monkeypatch):
    name, flat, pos, cpu = frame
    monkeypatch.setenv("ACN_CLASS0_MIN", "4" if wide else "1000000")   # 8 / 16 samples per point: above 4 they take k_shade<64>
    h = A.Handle(flat)
    gpu = h.render_positions(pos, linear=True)
    st = h.last_stages()
    h.close()
    err = np.abs(gpu - cpu)
    print(f"{name} wide={wide}: max |gpu - oracle| {err.max():.3e}, hard rays {st['hard_rays']:.0f}, probes {st['probe_rays']:.0f}")
    assert err.max() <= TOL, f"{name}: {(err > TOL).any(axis=1).sum()} of {len(pos)} pixels differ, max {err.max():.3e}"
    assert np.array_equal(eight_bit(flat, gpu), eight_bit(flat, cpu))
    # resumed records (k_shade's) and full ones (k_walk's probes) met in the hard-shadow queue
    assert st["hard_rays"] > 0 and st["probe_rays"] > 0, st


def test_overflow_retry_gives_the_same_bits(oracle, monkeypatch):
    """A chunk that does not fit its queues is halved and redone: the records written before the overflow are dropped
    with their words and the redone chunks write them again.  The frame of test_queue_overflow_retry_is_bit_identical
    (test_gpu_configs.py): the small frames above fit the smallest workspace."""
    flat = A.Scene.build("wine_glass", image_width=320, image_height=180, path_samples=64, direct_samples=50).flatten()
    pos = S.positions(flat)
    monkeypatch.setenv("ACN_LANES", "1")
    h = A.Handle(flat)
    ref = h.render_positions(pos, linear=True)
    st_ref = h.last_stages()
    h.close()
    assert st_ref["retries"] == 0 and st_ref["hard_rays"] > 0 and st_ref["probe_rays"] > 0, st_ref
    monkeypatch.setenv("ACN_WORKSPACE_MB", "48")       # 65 536 records per queue (the floor)
    monkeypatch.setenv("ACN_CHUNK", str(len(pos)))     # every position in one chunk
    h = A.Handle(flat)
    forced = h.render_positions(pos, linear=True)
    st = h.last_stages()
    h.close()
    print(f"retries {st['retries']:.0f}, chunks {st['chunks']:.0f}")
    assert st["retries"] > 0 and st["chunks"] > 1, st
    assert np.array_equal(forced, ref)
    # ... and on concurrent lanes, which hold their own copy of what the kernels are launched with: with room, and with
    # each lane's share of a small workspace
    for lanes, mb in (("3", None), ("2", "96")):
        monkeypatch.setenv("ACN_LANES", lanes)
        monkeypatch.delenv("ACN_WORKSPACE_MB") if mb is None else monkeypatch.setenv("ACN_WORKSPACE_MB", mb)
        monkeypatch.delenv("ACN_CHUNK", raising=False)
        if mb is not None:
            monkeypatch.setenv("ACN_CHUNK", str(len(pos)))
        h = A.Handle(flat)
        got = h.render_positions(pos, linear=True)
        stl = h.last_stages()
        h.close()
        assert (stl["retries"] > 0) == (mb is not None), stl
        assert np.array_equal(got, ref), f"{lanes} lanes, workspace {mb}"
    sample = np.arange(0, len(pos), 53)
    cpu = oracle.render_positions(flat, pos[sample], linear=True)
    assert np.abs(forced[sample] - cpu).max() <= TOL

"""The default lane plan and the lanes' stream order on the GPU, on wine_glass 320 x 180 at path_samples 64 / direct_samples 50: the
smallest shape at which three lanes run (acn_lanes_for_counts).

  - the frame does not depend on the plan: ACN_LANES unset, 1 and 6 give the same bits, and without ACN_LANES the call runs on
    acn_lanes_for_counts( ACN_DEFAULT_LANES, n, 64 ) lanes, each resolving its share once;
  - a _dev call on a caller's stream is ordered on that stream at both ends without a host wait in between: what the caller queued
    before it is read, what the caller queues after it sees the frame (render_lanes: the lanes wait for the caller's event, the
    caller's stream for the lanes');
  - chunks that are redone on the lanes: same bits, no host wait besides the one of every chunk run, one k_finalize per lane."""
import os
import re

import numpy as np
import pytest
import torch

import actinon_amd as A
import scenes_util as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LANE_TILE = 256


def default_lanes():
    text = open(os.path.join(os.path.dirname(HERE), "actinon_amd", "csrc", "acn_queueplan.h")).read()
    return int(re.search(r"#define\s+ACN_DEFAULT_LANES\s+(\d+)", text).group(1))


def lanes_for_counts(tun_lanes, n, path_samples):
    """acn_lanes_for_counts (acn_queueplan.h; compared with the header in tests/test_queueplan_cpu.py)"""
    lanes, work = tun_lanes, n * (path_samples + 1)
    while lanes > 1 and (n < lanes * 32 * LANE_TILE or work < lanes << 20):
        lanes -= 1
    return lanes


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def scene():
    """The scene, two sets of positions (pixel centres, and the same moved by a quarter pixel) and their frames on ONE lane: the
    reference of every test here, rendered once."""
    flat = A.Scene.build("wine_glass", image_width=320, image_height=180, path_samples=64, direct_samples=50).flatten()
    pos = S.positions(flat)
    pos2 = pos + 0.25
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ACN_LANES", "1")
        h = A.Handle(flat)
        ref, st = h.render_positions(pos, linear=True), h.last_stages()
        ref2 = h.render_positions(pos2, linear=True)
        h.close()
    assert st["retries"] == 0 and st["finalize_launches"] == 1
    assert ref.std() > 1e-3 and not np.array_equal(ref, ref2)
    for a in (pos, pos2, ref, ref2):
        a.setflags(write=False)
    return flat, pos, pos2, ref, ref2


@pytest.mark.parametrize("lanes", [None, "1", "6"], ids=["default", "one", "six"])
def test_frame_does_not_depend_on_the_lane_plan(scene, lanes, monkeypatch):
    flat, pos, _, ref, _ = scene
    if lanes is None:
        monkeypatch.delenv("ACN_LANES", raising=False)
    else:
        monkeypatch.setenv("ACN_LANES", lanes)
    for name in ("ACN_GRID", "ACN_SHADE_GRID", "ACN_WALK_GRID", "ACN_CHUNK", "ACN_WORKSPACE_MB"):
        monkeypatch.delenv(name, raising=False)
    h = A.Handle(flat)
    got, st = h.render_positions(pos, linear=True), h.last_stages()
    again, st2 = h.render_positions(pos, linear=True), h.last_stages()     # the warm handle: no learning pass, no host wait at the start
    h.close()
    want = lanes_for_counts(default_lanes() if lanes is None else int(lanes), len(pos), 64)
    print(f"ACN_LANES {lanes}: {want} lanes, finalize_launches {st['finalize_launches']:.0f} / {st2['finalize_launches']:.0f}, "
          f"chunks {st2['chunks']:.0f}, host_syncs {st2['host_syncs']:.0f}, retries {st['retries']:.0f} / {st2['retries']:.0f}")
    assert np.array_equal(got, ref) and np.array_equal(again, ref)
    assert st["retries"] == 0 and st2["retries"] == 0
    assert st["finalize_launches"] == want and st2["finalize_launches"] == want
    assert st["host_syncs"] == st["chunks"] and st2["host_syncs"] == st2["chunks"]


def test_dev_call_is_ordered_on_the_callers_stream_at_both_ends(scene, monkeypatch):
    """No host wait between: a device copy fills the position buffer, the call follows, a device copy of its output follows, a second
    call with other positions goes into a second buffer, ONE synchronisation ends the sequence."""
    flat, pos, pos2, ref, ref2 = scene
    monkeypatch.delenv("ACN_LANES", raising=False)
    n = len(pos)
    dev = torch.device("cuda", 0)
    src, src2 = torch.from_numpy(pos.copy()).to(dev), torch.from_numpy(pos2.copy()).to(dev)
    d_pos = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    out, out2, kept = (torch.zeros((n, 3), dtype=torch.float64, device=dev) for _ in range(3))
    h = A.Handle(flat)
    assert lanes_for_counts(default_lanes(), n, 64) > 1
    # (a cold handle learns first and waits while it does: the sequence runs on the warm one)
    h.render_positions_dev(src.data_ptr(), n, out.data_ptr(), linear=True)
    torch.cuda.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pos.copy_(src, non_blocking=True)
        h.render_positions_dev(d_pos.data_ptr(), n, out.data_ptr(), linear=True, stream=s.cuda_stream)
        kept.copy_(out, non_blocking=True)
        d_pos.copy_(src2, non_blocking=True)
        h.render_positions_dev(d_pos.data_ptr(), n, out2.data_ptr(), linear=True, stream=s.cuda_stream)
    s.synchronize()
    st = h.last_stages()
    got, got_kept, got2 = out.cpu().numpy(), kept.cpu().numpy(), out2.cpu().numpy()
    h.close()
    assert st["finalize_launches"] == lanes_for_counts(default_lanes(), n, 64)
    assert np.array_equal(got, ref) and np.array_equal(got_kept, ref)
    assert np.array_equal(got2, ref2)


def test_redone_chunks_on_the_lanes_add_no_host_wait(scene, monkeypatch):
    """The settings of test_queue_overflow_retry_is_bit_identical (tests/test_gpu_configs.py): two lanes, each with its share of a
    small workspace and a chunk that is too large for it.  The host waits once per chunk RUN: `chunks` counts the chunks that
    fitted and `retries` those that were run and redone, so "no wait besides a chunk's own" is host_syncs == chunks + retries
    (measured: 74 == 64 + 10; host_syncs == chunks is that statement for a call without retries, asserted above, and cannot hold
    with retries > 0).  A lane resolves its share once, behind its last chunk, and does not wait for that."""
    flat, pos, _, ref, _ = scene
    monkeypatch.setenv("ACN_LANES", "2")
    monkeypatch.setenv("ACN_WORKSPACE_MB", "96")
    monkeypatch.setenv("ACN_CHUNK", str(len(pos)))
    h = A.Handle(flat)
    got, st = h.render_positions(pos, linear=True), h.last_stages()
    h.close()
    print(f"retries {st['retries']:.0f}, chunks {st['chunks']:.0f}, host_syncs {st['host_syncs']:.0f}, finalize_launches {st['finalize_launches']:.0f}")
    assert st["retries"] > 0, st
    assert st["host_syncs"] == st["chunks"] + st["retries"], st
    assert st["finalize_launches"] == 2, st
    assert np.array_equal(got, ref)

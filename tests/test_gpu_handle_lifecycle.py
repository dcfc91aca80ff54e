"""The life cycle of a scene handle on the GPU: everything a handle and its runners own on the device (acn_handle.h, acn_devbuf.h)
goes when the handle is closed, nothing goes twice, and a handle made afterwards computes the same frame."""
import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
CYCLES = 4


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def one_cycle(flat, pos):
    """upload, one call of every kind that leaves a buffer on the handle or its runners, close -> ( the main-pass frame, W )"""
    import torch
    h = A.Handle(flat)
    frame = h.render_positions(pos, linear=True)                    # the whole main pass, on the lanes
    st = h.last_stages()
    assert st["finalize_launches"] == 3, st                         # three lanes ran: each owns a workspace, a stream, a thread
    h.render_positions(pos[:4096], linear=True)                     # the handle's own run; the lanes give their queues back
    assert h.last_stages()["finalize_launches"] == 1
    h.render_rays(h.camera_rays(pos), linear=True)                  # the ray check, the lanes' inputs as rays
    few = pos[:37]
    h.surface_positions(few)
    h.render_lens(few, linear=True, samples=3, aperture=0.15, focus=12.0)
    h.render_lens_stats(few, linear=True, samples=3, aperture=0.15, focus=12.0)
    small = A.main_pass_positions(9, 5)                             # a 9 x 5 frame: its records, and as many pixels of the frame above
    h.denoise(frame[:45].reshape(5, 9, 3), h.surface_positions(small, follow=True))
    key = np.linspace(0.0, 1.0, 2049)
    h.select_above(key, 0.5)
    h.key_histogram(key)
    n = len(pos)
    part = torch.empty((hip.acn_shard_tile_padded(n, 2), 3), dtype=torch.float64, device="cuda:0")
    h.render_main_pass_shard_dev(0, n, 1, 2, part.data_ptr(), linear=True)
    torch.cuda.synchronize()
    del part
    h.close()
    return frame, st["workspace_bytes"]


def test_four_handles_one_after_the_other_leave_nothing_behind(monkeypatch):
    """Four cycles of upload, calls, close on ACN_LANES=3, wine_glass 320 x 180 p64 d50 (the smallest shape at which three lanes run:
    tests/test_queueplan_cpu.py), never two handles alive.  Every scratch buffer of the handle and every buffer of its lanes exists
    when it is closed.  The frames of cycles 2 - 4 have the bits of cycle 1, and the free device memory after cycles 2 - 4 is not
    below the value after cycle 1 by more than W / 4, W the queue workspace of the first call: cycle 1 pays for code objects and
    whatever the runtime keeps, a workspace that is not released costs at least W per cycle, and a block freed twice ends the
    process.  (Small leaks are the business of tests/test_devbuf_cpu.py and of the reader.)"""
    import torch
    monkeypatch.setenv("ACN_LANES", "3")                            # (tunables are read at the upload)
    sc = A.Scene.build("wine_glass", image_width=320, image_height=180, path_samples=64, direct_samples=50)
    flat = sc.flatten()
    pos = S.positions(flat)
    first, w, free = None, None, []
    for cycle in range(CYCLES):
        frame, bytes_first_call = one_cycle(flat, pos)
        torch.cuda.empty_cache()
        free.append(torch.cuda.mem_get_info(0)[0])
        if cycle == 0:
            first, w = frame, bytes_first_call
        else:
            assert np.array_equal(frame, first), f"cycle {cycle + 1}"
    drops = [free[0] - f for f in free[1:]]
    print(f"W = {w:.0f} bytes; free after each cycle {free}; drops against cycle 1 {drops}")
    assert w > 0
    assert max(drops) <= w / 4, (drops, w)

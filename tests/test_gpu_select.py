"""Selecting positions by a key on the device (include/actinon_hip.h: acn_select_above*, acn_key_histogram*; k_select.hip) against the
numpy model tests/select_model.py, bit for bit: every size that crosses a boundary of a wave, a workgroup, a tile of any legal size
and a round of the scan of the tile counts; every pattern, threshold and capacity of the contract, with poison behind the results;
both sources of positions; a caller's stream; the host forms; the histogram; that the calls leave the renderer alone; and
tools/render_progressive.py with --select library and --rays-per-pass against its torch path."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
import select_model as SM
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ([1, 63, 64, 65, 255, 256, 257] + [2 ** k + d for k in range(9, 14) for d in (-1, 0, 1)] + [3 * 8192 + 5, 2 ** 20 + 3, 2 ** 22 + 1])
TILE = int(re.search(r"^#define ACN_SELECT_TILE (\d+)u", open(os.path.join(ROOT, "actinon_amd", "csrc", "acn_select_host.h")).read(), re.M).group(1))
WIDTHS = [1, 7, 1920]
SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.225073858507201e-308])


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def flat():
    return S.build("wine_glass_c2")[1]


@pytest.fixture(scope="module")
def h(flat):
    handle = A.Handle(flat)
    yield handle
    handle.close()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def sprinkled(rng, n):
    """keys uniform in [ 0, 1 ) with NaN, +-inf, -0.0 and denormals sprinkled in (about one entry in eight)"""
    key = rng.random(n)
    at = rng.integers(0, n, max(1, n // 8))
    key[at] = SPECIALS[rng.integers(0, len(SPECIALS), len(at))]
    return key


def patterns(rng, n):
    """( name, key, threshold ) of every pattern of the contract at this size"""
    ramp = np.arange(n, dtype=np.float64)
    mixed = sprinkled(rng, n)
    half = sprinkled(rng, n)
    finite = half[np.isfinite(half)]
    equal = float(np.sort(finite)[len(finite) // 2]) if len(finite) else 0.5   # a value equal to some key: strict >
    run = np.zeros(n)
    run[:TILE] = 1.0
    return [("all", rng.random(n) + 1.0, 0.5), ("all above -inf", np.where(np.isnan(mixed) | np.isneginf(mixed), 0.25, mixed), -np.inf),
            ("none above +inf", mixed, np.inf), ("none", rng.random(n), 1.0),
            ("only entry 0", (ramp == 0) * 1.0, 0.5), ("only entry n - 1", (ramp == n - 1) * 1.0, 0.5),
            ("alternating", ramp % 2, 0.5), ("random 1 %", mixed, 0.99), ("random 50 %, a threshold equal to a key", half, equal),
            ("everything but NaN", mixed, -np.inf), ("one tile, then none", run, 0.5)]


def as_bits(torch, t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("n", SIZES)
def test_select_has_the_models_bits(h, torch, n):
    """every pattern x every capacity x both sources of positions; out buffers of capacity + 64 entries filled with poison"""
    dev = torch.device("cuda", h.device)
    rng = np.random.default_rng(n)
    src = rng.random((n, 2)) * 1e3
    src[rng.integers(0, n, max(1, n // 16))] = [np.nan, -0.0]
    d_src = torch.from_numpy(src).to(dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    case = 0
    for name, key, threshold in patterns(rng, n):
        want_idx = SM.select(key, threshold)
        count = len(want_idx)
        if name.startswith("all"):
            assert count == n, name
        if name.startswith("none"):
            assert count == 0, name
        if name.startswith("only"):
            assert count == 1
        d_key = torch.from_numpy(key).to(dev)
        d_want_idx = torch.from_numpy(want_idx).to(dev)
        d_want_gather = d_src[d_want_idx]
        case += 1
        width, first = WIDTHS[case % 3], 3 + case
        d_want_raster = torch.from_numpy(SM.raster_positions(want_idx, width, first)).to(dev)
        for capacity in sorted({0, 1, max(count - 1, 0), count, count + 7}):
            m = min(count, capacity)
            for raster in (False, True):
                d_idx = torch.full((capacity + 64,), int(SM.POISON_INDEX), dtype=torch.int64, device=dev)
                d_pos = torch.full((capacity + 64, 2), float("nan"), dtype=torch.float64, device=dev)
                d_pos.view(torch.int64).fill_(int(np.array([SM.POISON_DOUBLE]).view(np.int64)[0]))
                d_count.fill_(-1)
                torch.cuda.synchronize(dev)
                pure = capacity == 0 and raster                                 # a pure count: no out buffers at all
                got = h.select_above_dev(d_key.data_ptr(), n, threshold, capacity, d_index_ptr=None if pure else d_idx.data_ptr(),
                                         d_pos_ptr=None if pure else d_pos.data_ptr(), d_src_pos_ptr=None if raster else d_src.data_ptr(),
                                         raster_width=width if raster else 0, raster_first=first if raster else 0, d_count_ptr=d_count.data_ptr())
                where = (name, n, capacity, raster)
                assert got == count and int(d_count.item()) == count, (where, got, int(d_count.item()), count)
                assert torch.equal(d_idx[:m], d_want_idx[:m]), where
                want_pos = (d_want_raster if raster else d_want_gather)[:m]
                assert torch.equal(as_bits(torch, d_pos[:m]), as_bits(torch, want_pos)), where
                assert bool((d_idx[m:] == int(SM.POISON_INDEX)).all()), where      # nothing at or beyond min( count, capacity )
                assert bool((as_bits(torch, d_pos[m:]) == int(np.array([SM.POISON_DOUBLE]).view(np.int64)[0])).all()), where


def test_raster_positions_are_the_tools_and_the_renderers(h, flat, torch):
    """without src_pos_xy and with raster_width 0 the positions are those of the scene's raster: the bits of main_pass_positions, of the
    tool's centres, and -- through acn_lens_rays without jitter and with aperture 0 against acn_camera_rays -- the positions whose rays
    acn_render_lens_stats_main_pass_dev casts"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_progressive as tool
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n = w * hh
    rng = np.random.default_rng(1)
    key = rng.random(n)
    idx, pos, count = h.select_above(key, 0.5)
    assert count == len(idx) and np.array_equal(idx, SM.select(key, 0.5))
    want = A.main_pass_positions(w, hh)[idx]
    assert np.array_equal(pos.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(pos, tool.centres(torch.from_numpy(idx), w).numpy())
    rays = h.lens_rays(pos, samples=1, jitter=False, aperture=0.0)
    assert np.array_equal(rays.reshape(-1, 6).view(np.uint64), h.camera_rays(want).view(np.uint64))
    # another raster and a first pixel: the tool's centres( idx + first, W )
    for width in WIDTHS:
        first = 1000003
        idx2, pos2, _ = h.select_above(key, 0.5, raster_width=width, raster_first=first)
        assert np.array_equal(idx2, idx)
        assert np.array_equal(pos2, tool.centres(torch.from_numpy(idx + first), width).numpy())
        assert np.array_equal(pos2, SM.raster_positions(idx, width, first))


@pytest.mark.parametrize("n", [1, 257, TILE + 1, 2 ** 20 + 3])
def test_a_callers_stream_and_the_host_form(h, torch, n):
    dev = torch.device("cuda", h.device)
    rng = np.random.default_rng(n + 1)
    key, src = sprinkled(rng, n), rng.random((n, 2))
    want_idx, want_pos, count = SM.select_above(key, 0.5, n, src_pos=src)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_key = torch.from_numpy(key).to(dev, non_blocking=False)
        d_src = torch.from_numpy(src).to(dev)
        d_idx = torch.full((n,), -1, dtype=torch.int64, device=dev)
        d_pos = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
        d_count = torch.full((1,), -1, dtype=torch.int64, device=dev)
        d_hist = torch.full((SM.WORDS,), 99, dtype=torch.int64, device=dev)
        # no host count: the call returns without a synchronisation; the results are read after the caller's own
        assert h.select_above_dev(d_key.data_ptr(), n, 0.5, n, d_index_ptr=d_idx.data_ptr(), d_pos_ptr=d_pos.data_ptr(), d_src_pos_ptr=d_src.data_ptr(),
                                  d_count_ptr=d_count.data_ptr(), want_count=False, stream=stream.cuda_stream) is None
        h.key_histogram_dev(d_key.data_ptr(), n, d_hist.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert int(d_count.item()) == count
        assert np.array_equal(d_idx[:count].cpu().numpy(), want_idx)
        assert np.array_equal(d_pos[:count].cpu().numpy().view(np.uint64), want_pos.view(np.uint64))
        assert bool((d_idx[count:] == -1).all()) and bool((d_pos[count:] == -1.0).all())
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint64), SM.histogram(key))
        # with a host count the call synchronises the stream itself
        d_idx.fill_(-1)
        assert h.select_above_dev(d_key.data_ptr(), n, 0.5, n, d_index_ptr=d_idx.data_ptr(), stream=stream.cuda_stream) == count
        assert np.array_equal(d_idx[:count].cpu().numpy(), want_idx)
    # the host form equals the device form, also when the list is cut, and writes nothing behind it
    idx, pos, got = h.select_above(key, 0.5, src_pos=src)
    assert got == count and np.array_equal(idx, want_idx) and np.array_equal(pos.view(np.uint64), want_pos.view(np.uint64))
    cap = max(count - 1, 0)
    idx, pos, got = h.select_above(key, 0.5, src_pos=src, capacity=cap)
    assert got == count and np.array_equal(idx, want_idx[:cap]) and np.array_equal(pos.view(np.uint64), want_pos[:cap].view(np.uint64))
    out_idx = np.full(cap + 8, 77, dtype=np.int64)
    out_pos = np.full((cap + 8, 2), 7.25)
    total = C.c_uint64(0)
    p = A.Handle.select_params(0.5, cap + 8)
    A.check(hip.acn_select_above(h.h, key.ctypes.data, n, C.byref(p), src.ctypes.data, out_idx.ctypes.data, out_pos.ctypes.data, C.byref(total)), "acn_select_above")
    m = min(count, cap + 8)
    assert total.value == count and np.array_equal(out_idx[:m], want_idx[:m]) and (out_idx[m:] == 77).all() and (out_pos[m:] == 7.25).all()
    assert h.select_above(key, 0.5, capacity=0)[2] == count                    # a pure count
    assert h.select_above(np.zeros(0), 0.5)[2] == 0                            # n == 0
    assert np.array_equal(h.key_histogram(key), SM.histogram(key)) and int(h.key_histogram(np.zeros(0)).sum()) == 0


@pytest.fixture(scope="module")
def wine48(tmp_path_factory):
    """the wine glass at 48 x 27, K = 2: the flattened scene on disk and the noise after pass 0"""
    w, hh, K = 48, 27, 2
    fl = A.Scene.build("wine_glass", **dict(S.SMALL["wine_glass_c2"][1], image_width=w, image_height=hh)).flatten()
    path = tmp_path_factory.mktemp("wine48") / "scene.npz"
    fl.save(str(path))
    hd = A.Handle(fl)
    noise0 = hd.render_lens_stats(S.positions(fl), linear=True, samples=K, jitter=True, seed=0)[1].noise
    hd.close()
    return str(path), noise0, (w, hh, K)


@pytest.mark.parametrize("n", SIZES)
def test_histogram_is_exact(h, torch, n):
    dev = torch.device("cuda", h.device)
    rng = np.random.default_rng(n + 2)
    keys = [sprinkled(rng, n) * 2.0 ** rng.integers(-50, 8, n), rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64),
            np.full(n, 0.03125)]                                                # spread over the bins; raw bit patterns; one crowded bin
    d_hist = torch.full((SM.WORDS,), 12345, dtype=torch.int64, device=dev)      # overwritten, not added to: also by the second call
    for key in keys:
        d_key = torch.from_numpy(key).to(dev)
        torch.cuda.synchronize(dev)
        h.key_histogram_dev(d_key.data_ptr(), n, d_hist.data_ptr())
        got = d_hist.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, SM.histogram(key)) and int(got.sum()) == n
    assert int(got[SM.key_bin(np.array([0.03125]))[0]]) == n


def test_histogram_of_a_real_noise_map_and_its_threshold(h, wine48):
    _, noise0, (w, hh, K) = wine48
    hist = h.key_histogram(noise0)
    assert np.array_equal(hist, SM.histogram(noise0)) and int(hist.sum()) == w * hh
    for budget in (0, 1, w * hh // 4, w * hh // 2, w * hh):
        t = A.key_hist_threshold(hist, budget)
        assert t == SM.threshold(hist, budget)
        idx, _, count = h.select_above(noise0, t)
        assert count <= budget and np.array_equal(idx, SM.select(noise0, t))


def test_refusals_write_nothing(h, torch):
    dev = torch.device("cuda", h.device)
    d_key = torch.arange(8, dtype=torch.float64, device=dev)
    d_idx = torch.full((8,), 77, dtype=torch.int64, device=dev)
    d_pos = torch.full((8, 2), 7.25, dtype=torch.float64, device=dev)
    d_count = torch.full((1,), 77, dtype=torch.int64, device=dev)
    d_hist = torch.full((SM.WORDS,), 77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    sharded = abi.RenderOpts()
    sharded.struct_size, sharded.shard_world = C.sizeof(abi.RenderOpts), 2
    total = C.c_uint64(77)

    def call(word, key=d_key.data_ptr(), n=8, prm=None, null_prm=False, idx=d_idx.data_ptr(), pos=d_pos.data_ptr(), opts=o):
        q = A.Handle.select_params(0.5, 8) if prm is None else prm
        st = hip.acn_select_above_dev(h.h, key, n, None if null_prm else C.byref(q), None, idx, pos, d_count.data_ptr(), C.byref(total), C.byref(opts))
        assert st == abi.ACN_ERR_ARG and word.encode() in hip.acn_last_error(), (word, st, hip.acn_last_error())

    def prm(**kw):
        q = A.Handle.select_params(0.5, 8)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    call("key", key=None)
    call("2^31", n=2 ** 31 + 1)
    call("acn_select_params", null_prm=True)
    call("struct_size", prm=prm(struct_size=12))
    call("flags", prm=prm(flags=4))
    call("NaN", prm=prm(threshold=float("nan")))
    call("capacity", idx=None, pos=None)
    call("sharded", opts=sharded)
    call("align", idx=d_idx.data_ptr() + 4)
    call("2^52", prm=prm(raster_first=2 ** 52))
    assert hip.acn_key_histogram_dev(h.h, None, 8, d_hist.data_ptr(), C.byref(o)) == abi.ACN_ERR_ARG and b"key" in hip.acn_last_error()
    assert hip.acn_key_histogram_dev(h.h, d_key.data_ptr(), 8, None, C.byref(o)) == abi.ACN_ERR_ARG and b"out_hist" in hip.acn_last_error()
    assert hip.acn_key_histogram_dev(h.h, d_key.data_ptr(), 2 ** 31 + 1, d_hist.data_ptr(), C.byref(o)) == abi.ACN_ERR_ARG and b"2^31" in hip.acn_last_error()
    assert hip.acn_key_histogram_dev(h.h, d_key.data_ptr(), 8, d_hist.data_ptr(), C.byref(sharded)) == abi.ACN_ERR_ARG and b"sharded" in hip.acn_last_error()
    torch.cuda.synchronize(dev)
    assert bool((d_idx == 77).all()) and bool((d_pos == 7.25).all()) and int(d_count.item()) == 77 and bool((d_hist == 77).all()) and total.value == 77
    # n == 0: ACN_OK, both counts 0
    assert h.select_above_dev(None, 0, 0.5, 8, d_index_ptr=d_idx.data_ptr(), d_count_ptr=d_count.data_ptr()) == 0
    assert int(d_count.item()) == 0 and bool((d_idx == 77).all())


def test_the_calls_leave_the_renderer_alone(flat, wine48):
    """the 25 values of acn_last_stage_ms and the bits of a frame, before and after a select call and a histogram call"""
    pos = S.positions(flat)
    hd = A.Handle(flat)
    hd.render_positions(pos, linear=True)                                       # a warm handle
    before = hd.render_positions(pos, linear=True)
    stages = hd.last_stages()
    assert len(stages) == 25 and stages["retries"] == 0
    key = np.random.default_rng(5).random(3 * TILE + 5)
    for _ in range(2):
        idx, _, count = hd.select_above(key, 0.5)
        assert count == len(idx) == int((key > 0.5).sum())
        assert int(hd.key_histogram(key).sum()) == len(key)
        assert hd.last_stages() == stages                                       # [ 23 ] and [ 24 ], the workspace, included
    after = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0 and hd.last_stages()["workspace_allocs"] == stages["workspace_allocs"]
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    hd.close()


def test_the_progressive_tool_selects_through_the_library(wine48, tmp_path):
    """48 x 27, K = 2, three passes, T the median noise after pass 0.  --select library: the records, the final noise and the rays of
    every pass are those of the torch path, bit for bit.  --rays-per-pass B, B half of pass 0's rays: every later pass casts at most B
    rays and its pixels are the model's for max( T, T_B )."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_progressive as tool
    scene, noise0, (w, hh, K) = wine48
    n, P = w * hh, 3
    target = float(np.median(noise0))
    assert np.isfinite(target) and target > 0
    quiet = lambda *_: None
    seen = {"torch": [], "library": [], "budget": []}

    def record(into):
        return lambda p, t, idx, d_noise: into.append((p, t, idx.cpu().numpy().copy(), d_noise.cpu().numpy().copy()))

    frame_t, rec_t, noise_t, rays_t = tool.render(A.Flat.load(scene), K, P, target, log=quiet, on_pass=record(seen["torch"]))
    frame_l, rec_l, noise_l, rays_l = tool.render(A.Flat.load(scene), K, P, target, log=quiet, select_mode="library", on_pass=record(seen["library"]))
    assert rays_l == rays_t and len(rays_t) == P and rays_t[1] > 0
    assert np.array_equal(rec_l.view(np.uint64), rec_t.view(np.uint64)) and np.array_equal(noise_l.view(np.uint64), noise_t.view(np.uint64))
    assert np.array_equal(frame_l, frame_t)
    assert np.array_equal(seen["torch"][0][3].view(np.uint64), noise0.view(np.uint64))
    for a, b in zip(seen["library"], seen["torch"]):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[2], SM.select(b[3], target))
    B = rays_t[0] // 2
    frame_b, rec_b, noise_b, rays_b = tool.render(A.Flat.load(scene), K, P, target, log=quiet, select_mode="library", rays_per_pass=B,
                                                  on_pass=record(seen["budget"]))
    assert rays_b[0] == n * K and len(rays_b) == P and all(0 < r <= B for r in rays_b[1:])
    for (p, t, idx, noise), r in zip(seen["budget"], rays_b[1:]):
        want_t = max(target, SM.threshold(SM.histogram(noise), B // K))
        assert t == want_t
        assert np.array_equal(idx, SM.select(noise, want_t)) and r == len(idx) * K
    # the command line takes both options and writes that frame
    out = tmp_path / "b.pnm"
    tool.main([scene, str(out), "--samples", str(K), "--passes", str(P), "--target-noise", repr(target), "--select", "library", "--rays-per-pass", str(B)])
    from render_aovs import read_pnm
    assert np.array_equal(read_pnm(str(out)), frame_b)

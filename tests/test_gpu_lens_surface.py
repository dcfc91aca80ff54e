"""Lens surface records on the GPU (acn_surface_reduce*, acn_surface_lens*; include/actinon_hip.h) against the numpy model of
tests/lens_surface_model.py, bit for bit (test_lens_surface_cpu.py checks the model); the calls' contracts (slices, streams, lanes,
refusals, the renderer left alone); the aggregate record through the filter; what lens guides buy a depth-of-field frame against a
converged one; and tools/render_progressive.py --guides."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import lens_surface_model as R
import scenes_util as S
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = dict(aperture=0.15, focus=12.0, jitter=True)
W, H = 96, 54
# K = 1; the edges of a lens slice's tiles (64 x 16); then either side of SURF_TILE_POS = 16 positions and SURF_TILE_K = 16 samples of
# k_surface_reduce, and two tiles each way
SHAPES = [(1, 1), (1, 2), (63, 5), (64, 16), (65, 17), (130, 33), (15, 15), (16, 15), (17, 16), (31, 31), (32, 32), (33, 17)]


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
def edge_pos(h, flat):
    """the 64 edge positions of the pinhole FOLLOW frame (lens_surface_model.edge_positions), then positions spread over the frame"""
    pos = S.positions(flat)
    idx, count = R.edge_positions(h.surface_positions(pos, follow=True).raw, W, H)
    assert len(idx) == 64 and count >= 128, (len(idx), count)
    rest = np.setdiff1d(np.arange(len(pos)), idx)
    out = np.concatenate([pos[idx], pos[rest[:: len(rest) // 80][:80]]])
    out.setflags(write=False)
    return out


def assert_same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def ray_records(h, pos, follow, **lens):
    """acn_lens_rays -> acn_surface_rays: the K records of every position [n,K,16]"""
    rays = h.lens_rays(pos, **lens)
    n, K = rays.shape[:2]
    return h.surface_rays(rays.reshape(n * K, 6), follow=follow).raw.reshape(n, K, 16)


@pytest.mark.parametrize("name", list(R.hand_made()))
def test_reduce_on_hand_made_records(h, detmath_cpu, name):
    import torch
    rec, _ = R.hand_made()[name]
    want = R.reduce(detmath_cpu, rec)
    assert_same_bits(h.surface_reduce(rec).raw, want)
    # device buffers on a caller's stream; one record behind the last stays untouched
    n, K = rec.shape[:2]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rec = torch.from_numpy(rec).to("cuda")
        d_out = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
        h.surface_reduce_dev(d_rec.data_ptr(), n, K, d_out.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    got = d_out.cpu().numpy()
    assert_same_bits(got[:n], want)
    assert np.isnan(got[n]).all()
    assert_same_bits(d_rec.cpu().numpy(), rec)


def test_all_hand_made_positions_in_one_call(h, detmath_cpu):
    """the same records as neighbours in one workgroup: positions that need 1, 2, 3 and 5 rounds of the class table side by side"""
    cases = R.hand_made()
    rec = np.concatenate([cases["9 / 17 / K classes at K = 33"][0]] * 5 + [np.repeat(cases["one class"][0], 7, axis=1)[:, :33]])
    perm = np.random.default_rng(2).permutation(len(rec))
    assert_same_bits(h.surface_reduce(rec[perm]).raw, R.reduce(detmath_cpu, rec)[perm])


@pytest.mark.parametrize("follow", [False, True])
def test_lens_call_is_rays_surface_reduce(h, detmath_cpu, edge_pos, follow):
    mixed = 0
    for n, K in SHAPES:
        pos = edge_pos[:n]
        assert len(pos) == n
        lens = dict(LENS, samples=K, seed=0)
        rec = ray_records(h, pos, follow, **lens)
        want = R.reduce(detmath_cpu, rec)
        assert_same_bits(h.surface_reduce(rec).raw, want)
        got = h.surface_lens(pos, follow=follow, **lens)
        assert_same_bits(got.raw, want)
        assert (got.coverage > 0).all() and (got.coverage <= 1).all()
        mixed += int((got.coverage < 1).sum())
    assert mixed >= 100                                                       # (the edge positions are edge positions)


@pytest.mark.parametrize("lanes", [None, "1"])
def test_slices_and_the_main_pass_on_a_callers_stream(monkeypatch, flat, lanes):
    """600 positions, K = 4, 1024 rays per slice: three slices, the last one short; the main-pass form on a torch stream of the
    caller's against the position form"""
    import torch
    if lanes:
        monkeypatch.setenv("ACN_LANES", lanes)
    else:
        monkeypatch.delenv("ACN_LANES", raising=False)
    allpos = S.positions(flat)
    pos = allpos[::8][:600].copy()
    lens = dict(LENS, samples=4, seed=3)
    monkeypatch.setenv("ACN_LENS_SLICE_RAYS", "1024")
    sliced = A.Handle(flat)                                                 # (tunables are read at the upload)
    monkeypatch.delenv("ACN_LENS_SLICE_RAYS")
    one = A.Handle(flat)
    want = one.surface_lens(pos, follow=True, **lens).raw
    assert_same_bits(sliced.surface_lens(pos, follow=True, **lens).raw, want)
    assert_same_bits(one.surface_reduce(ray_records(one, pos, True, **lens)).raw, want)
    first, count = 1000, 700
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pos = torch.from_numpy(allpos[first:first + count]).to("cuda")
        a = torch.full((count + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
        b = torch.full((count + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
        for follow in (False, True):
            sliced.surface_lens_main_pass_dev(first, count, a.data_ptr(), follow=follow, stream=s.cuda_stream, **lens)
            one.surface_lens_dev(d_pos.data_ptr(), count, b.data_ptr(), follow=follow, stream=s.cuda_stream, **lens)
            s.synchronize()
            assert torch.equal(a[:count], b[:count]) and bool(torch.isnan(a[count]).all()) and bool(torch.isnan(b[count]).all()), follow
            assert_same_bits(a[:count].cpu().numpy(), one.surface_lens(allpos[first:first + count], follow=follow, **lens).raw)
    sliced.close()
    one.close()


def test_records_do_not_depend_on_wave_neighbours(h, edge_pos):
    pos = edge_pos[:130]
    lens = dict(LENS, samples=5)
    plain = h.surface_lens(pos, follow=True, **lens).raw
    perm = np.random.default_rng(1).permutation(130)
    assert_same_bits(h.surface_lens(pos[perm], follow=True, **lens).raw, plain[perm])
    assert_same_bits(h.surface_lens(pos[77:78], follow=True, **lens).raw, plain[77:78])
    padded = np.concatenate([edge_pos[130:137], pos[40:60], edge_pos[137:140]])
    assert_same_bits(h.surface_lens(padded, follow=True, **lens).raw[7:27], plain[40:60])


def test_one_sample_is_that_sample(h, edge_pos):
    """K = 1: coverage 1 everywhere, and the record is the record of acn_surface_rays( acn_lens_rays ) -- the rays behind
    acn_render_lens_stats with the same parameters and seed"""
    for follow in (False, True):
        lens = dict(LENS, samples=1, seed=4)
        got = h.surface_lens(edge_pos, follow=follow, **lens)
        rec = ray_records(h, edge_pos, follow, **lens)[:, 0]
        assert (got.coverage == 1.0).all()
        assert (got.hit == (rec[:, 0] < np.inf)).all() and got.hit.any()
        assert follow == (not got.hit.all())                                  # (the first surface is always there; a followed ray may leave)
        assert_same_bits(got.raw[:, :15], rec[:, :15])


def test_pinhole_identity(h, edge_pos):
    for follow in (False, True):
        got = h.surface_lens(edge_pos, follow=follow, samples=1)
        want = h.surface_positions(edge_pos, follow=follow)
        assert_same_bits(got.raw[:, :15], want.raw[:, :15])
        assert (want.coverage == 0).all() and (got.coverage == 1.0).all()
        # several samples of a closed aperture without jitter are one sample several times: the means of equal numbers
        four = h.surface_lens(edge_pos, follow=follow, samples=4)
        assert (four.coverage == 1.0).all()
        assert_same_bits(four.raw[:, [0, 7, 8, 12, 13, 14]], want.raw[:, [0, 7, 8, 12, 13, 14]])


def test_the_calls_leave_the_renderer_alone(flat, edge_pos):
    pos = S.positions(flat)
    hd = A.Handle(flat)
    hd.render_positions(pos, linear=True)                                   # a warm handle
    before = hd.render_positions(pos, linear=True)
    stages = hd.last_stages()
    assert stages["retries"] == 0
    raw = (C.c_double * 25)()
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    raw_before = list(raw)
    counters = hd.last_counters_raw(10)
    kernel_ms = hd.last_kernel_ms()
    surf = hd.surface_lens(pos, follow=True, samples=4, **LENS)
    hd.surface_lens(edge_pos, samples=33, **LENS)
    hd.surface_reduce(np.stack([surf.raw[:100], surf.raw[100:200]], axis=1))
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    assert list(raw) == raw_before                                          # [ 23 ], [ 24 ] included: nothing of the workspace moved
    assert list(hd.last_counters_raw(10)) == list(counters) and hd.last_kernel_ms() == kernel_ms
    after = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    assert np.array_equal(before, after)
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    assert list(raw)[23:25] == raw_before[23:25]
    assert_same_bits(hd.surface_lens(pos, follow=True, samples=4, **LENS).raw, surf.raw)
    hd.close()


def test_refusals_leave_the_output_untouched(flat, edge_pos):
    """Every ACN_ERR_ARG of the section: the status, acn_last_error, and not one word written, on host and device buffers; then the
    handle still works"""
    import torch
    pos = edge_pos[:40].copy()
    n, K = len(pos), 4
    h = A.Handle(flat)
    good = A.Handle.lens_params(samples=K, aperture=0.1, focus=12.0)
    o = h._plain_opts(False, None)
    rec = np.ascontiguousarray(ray_records(h, pos, True, samples=K, aperture=0.1, focus=12.0))
    d_pos = torch.from_numpy(pos).to("cuda")
    d_rec = torch.from_numpy(rec).to("cuda")
    d_out = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
    out = np.full((n + 1, 16), np.nan)
    torch.cuda.synchronize()

    def refused(table, word):
        for name, call in table.items():
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(out).all() and bool(torch.isnan(d_out).all()), name

    def lens_calls(handle, p, opts, mode=abi.ACN_SURF_FOLLOW, hp=pos.ctypes.data, dp=None, ho=None, do=None, first=0):
        dp = d_pos.data_ptr() if dp is None else dp
        ho = out.ctypes.data if ho is None else ho
        do = d_out.data_ptr() if do is None else do
        ref = C.byref(p) if p is not None else None
        return {"surface_lens": lambda: hip.acn_surface_lens(handle, hp, n, ref, mode, ho, C.byref(opts)),
                "surface_lens_dev": lambda: hip.acn_surface_lens_dev(handle, dp, n, ref, mode, do, C.byref(opts)),
                "surface_lens_main_pass_dev": lambda: hip.acn_surface_lens_main_pass_dev(handle, first, n, ref, mode, do, C.byref(opts))}

    def reduce_calls(handle, opts, k=K, hr=rec.ctypes.data, dr=None, ho=None, do=None):
        dr = d_rec.data_ptr() if dr is None else dr
        ho = out.ctypes.data if ho is None else ho
        do = d_out.data_ptr() if do is None else do
        return {"surface_reduce": lambda: hip.acn_surface_reduce(handle, hr, n, k, ho, C.byref(opts)),
                "surface_reduce_dev": lambda: hip.acn_surface_reduce_dev(handle, dr, n, k, do, C.byref(opts))}

    only = lambda table, *names: {k: v for k, v in table.items() if k in names}
    # a null handle, or a null buffer with n > 0
    refused(lens_calls(None, good, o), "handle")
    refused(reduce_calls(None, o), "handle")
    refused(only(lens_calls(h.h, good, o, hp=None), "surface_lens"), "null")
    refused({"dev": lambda: hip.acn_surface_lens_dev(h.h, None, n, C.byref(good), 1, d_out.data_ptr(), C.byref(o))}, "null")
    refused({"host out": lambda: hip.acn_surface_lens(h.h, pos.ctypes.data, n, C.byref(good), 1, None, C.byref(o)),
             "dev out": lambda: hip.acn_surface_lens_dev(h.h, d_pos.data_ptr(), n, C.byref(good), 1, None, C.byref(o)),
             "main out": lambda: hip.acn_surface_lens_main_pass_dev(h.h, 0, n, C.byref(good), 1, None, C.byref(o))}, "null")
    refused({"host records": lambda: hip.acn_surface_reduce(h.h, None, n, K, out.ctypes.data, C.byref(o)),
             "dev records": lambda: hip.acn_surface_reduce_dev(h.h, None, n, K, d_out.data_ptr(), C.byref(o)),
             "host out": lambda: hip.acn_surface_reduce(h.h, rec.ctypes.data, n, K, None, C.byref(o)),
             "dev out": lambda: hip.acn_surface_reduce_dev(h.h, d_rec.data_ptr(), n, K, None, C.byref(o))}, "null")
    # K == 0 or K > 4096
    refused(reduce_calls(h.h, o, k=0), "K 0")
    refused(reduce_calls(h.h, o, k=4097), "4097")
    # everything the lens refuses
    small_struct = A.Handle.lens_params(samples=K, aperture=0.1, focus=12.0)
    small_struct.struct_size = 3
    flags = A.Handle.lens_params(samples=K, aperture=0.1, focus=12.0)
    flags.flags = 2
    lp = A.Handle.lens_params
    for word, p in (("samples", lp(samples=4097, aperture=0.1, focus=12.0)), ("flags", flags), ("struct_size", small_struct),
                    ("aperture", lp(samples=K, aperture=-0.1, focus=12.0)), ("aperture", lp(samples=K, aperture=float("nan"), focus=12.0)),
                    ("focus", lp(samples=K, aperture=0.1, focus=0.0)), ("focus", lp(samples=K, aperture=0.1, focus=float("inf")))):
        refused(lens_calls(h.h, p, o), word)
    # an unknown mode; shard_world > 1
    refused(lens_calls(h.h, good, o, mode=2), "mode")
    world2 = h._plain_opts(False, None)
    world2.shard_world = 2
    refused(lens_calls(h.h, good, world2), "sharded")
    refused(reduce_calls(h.h, world2), "sharded")
    # buffers that are not 16-byte aligned
    refused(only(lens_calls(h.h, good, o, dp=d_pos.data_ptr() + 8), "surface_lens_dev"), "align")
    refused(only(lens_calls(h.h, good, o, do=d_out.data_ptr() + 8), "surface_lens_dev", "surface_lens_main_pass_dev"), "align")
    refused(only(reduce_calls(h.h, o, dr=d_rec.data_ptr() + 8), "surface_reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, do=d_out.data_ptr() + 8), "surface_reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, ho=out.ctypes.data + 8), "surface_reduce"), "align")
    # a pixel range outside the image
    refused(only(lens_calls(h.h, good, o, first=W * H - n + 1), "surface_lens_main_pass_dev"), "outside")
    # an open aperture needs the scene's focal length
    nofocal = A.Scene.build("wine_glass", **dict(S.SMALL["wine_glass_c2"][1], camera_focal_length=0.0)).flatten()
    hn = A.Handle(nofocal)
    refused(lens_calls(hn.h, good, o), "focal")
    hn.close()
    # n == 0 is ACN_OK and writes nothing, a null buffer included
    for call in (lambda: hip.acn_surface_lens_dev(h.h, None, 0, C.byref(good), 1, None, C.byref(o)),
                 lambda: hip.acn_surface_lens_main_pass_dev(h.h, 5, 0, C.byref(good), 1, d_out.data_ptr(), C.byref(o)),
                 lambda: hip.acn_surface_lens(h.h, None, 0, None, 0, None, None),
                 lambda: hip.acn_surface_reduce_dev(h.h, None, 0, K, None, C.byref(o)),
                 lambda: hip.acn_surface_reduce(h.h, None, 0, 1, out.ctypes.data, None)):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert np.isnan(out).all() and bool(torch.isnan(d_out).all())
    # and the handle works
    assert_same_bits(h.surface_lens(pos, follow=True, samples=K, aperture=0.1, focus=12.0).raw, h.surface_reduce(rec).raw)
    h.close()


@pytest.fixture(scope="module")
def frame(flat):
    """wine_glass_c2 96 x 54 through the lens at K = 8, seed 0: the statistics records, the aggregate and the pinhole FOLLOW records"""
    pos = S.positions(flat)
    hd = A.Handle(flat)
    lens = dict(LENS, samples=8, seed=0)
    st = hd.render_lens_stats(pos, linear=True, **lens)[1].raw
    agg = hd.surface_lens(pos, follow=True, **lens).raw
    pin = hd.surface_positions(pos, follow=True).raw
    hd.close()
    for a in (st, agg, pin):
        a.setflags(write=False)
    return st, agg, pin


def test_the_filter_takes_the_aggregate_record(h, detmath_cpu, flat, frame):
    """acn_denoise_stats and acn_denoise on aggregate records have denoise_model's bits: the filter reads doubles 0 .. 13 and is as it was"""
    st, agg, _ = frame
    bg = np.array(flat.params.background_color[:])
    assert (agg[:, 15] > 0).all() and (agg[:, 15] < 1).any()
    for params in (dict(), dict(iterations=2, normal_power_log2=3, demodulate=False)):
        assert_same_bits(h.denoise_stats(st, agg, W, H, **params), T.denoise_stats(detmath_cpu, st, agg, W, H, bg, **params))
    mean = st[:, 1:4].reshape(H, W, 3)
    assert_same_bits(h.denoise(mean, agg, iterations=3), D.denoise(detmath_cpu, mean, agg, iterations=3))
    # [ 14 ] and [ 15 ] are not read
    other = agg.copy()
    other[:, 14:16] = 0.0
    assert_same_bits(h.denoise_stats(st, other, W, H), h.denoise_stats(st, agg, W, H))


def test_quality_against_a_converged_frame(flat, frame):
    """Gate: on a 96 x 54 wine_glass_c2 frame of K = 8 lens samples (aperture 0.15, focus 12, jitter, seed 0) the MSE of
    acn_denoise_stats guided by the aggregate FOLLOW records -- linear, over the pixels filterable under both guide sets, against a
    K = 256 frame of the same lens and seed 9 taken as converged -- is below the MSE of the unfiltered K = 8 mean.  Recorded, not
    gated: the same with pinhole FOLLOW guides, and both with the pixels of coverage below 0.75 taken out of the filter.
    Seen on an MI355X, 5127 pixels: raw 1.202e-3; lens guides 6.82e-4 (0.567 of raw); pinhole guides 6.64e-4 (0.553); without the 102
    pixels of coverage below 0.75: lens 6.96e-4 (0.579), pinhole 6.98e-4 (0.581).  167 pixels have a coverage below 1: at this aperture
    the lens guides pass the gate and are no gain in MSE over the pinhole guides (profiles/r11/NOTES.md)."""
    st, agg, pin = frame
    pos = S.positions(flat)
    hd = A.Handle(flat)
    ref = hd.render_lens(pos, linear=True, **dict(LENS, samples=256, seed=9)).reshape(H, W, 3)
    mean = st[:, 1:4].reshape(H, W, 3)

    def low_out(rec):                                                       # --min-coverage 0.75 of tools/render_progressive.py
        r = rec.copy()
        r[r[:, 15] < 0.75, 0] = np.inf
        return r

    pin_cov = pin.copy()
    pin_cov[:, 15] = agg[:, 15]                                             # the same pixels leave the filter under either guide set
    out = {"lens": hd.denoise_stats(st, agg, W, H), "pinhole": hd.denoise_stats(st, pin, W, H),
           "lens, coverage >= 0.75": hd.denoise_stats(st, low_out(agg), W, H),
           "pinhole, coverage >= 0.75": hd.denoise_stats(st, low_out(pin_cov), W, H)}
    hd.close()
    ok = np.ones(W * H, bool)
    for rec in (agg, pin):
        ok &= D.filterable(rec, mean.reshape(-1, 3) / D.albedo(rec))
    ok = ok.reshape(H, W)
    assert ok.mean() > 0.5
    mse = lambda x: float(np.mean((x[ok] - ref[ok]) ** 2))
    e_raw = mse(mean)
    line = f"wine_glass_c2 96x54 K=8 lens vs K=256: linear mse over {int(ok.sum())} pixels filterable under both guide sets: raw {e_raw:.4e}"
    for name, img in out.items():
        line += f"  {name} {mse(img):.4e} ({mse(img) / e_raw:.3f} of raw)"
    print(line + f"  [{int((agg[:, 15] < 0.75).sum())} pixels of coverage < 0.75, {int((agg[:, 15] < 1).sum())} < 1]")
    assert mse(out["lens"]) < e_raw, (mse(out["lens"]), e_raw)


def test_the_progressive_tool_guides(tmp_path):
    """--guides pinhole writes the bytes of no option; --guides lens with an open aperture runs and differs"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_progressive as tool
    w, hh, K = 48, 27, 4
    sc = A.Scene.build("wine_glass", **dict(S.SMALL["wine_glass_c2"][1], image_width=w, image_height=hh))
    scene = tmp_path / "scene.npz"
    sc.flatten().save(str(scene))
    names = {}
    base = [str(scene), None, "--samples", str(K), "--passes", "2", "--target-noise", "0.05", "--denoise", "--aperture", "0.15", "--focus", "12"]
    for key, extra in (("none", []), ("pinhole", ["--guides", "pinhole"]), ("lens", ["--guides", "lens"]),
                       ("lens75", ["--guides", "lens", "--min-coverage", "0.75"])):
        names[key] = tmp_path / (key + ".pnm")
        args = list(base)
        args[1] = str(names[key])
        tool.main(args + extra)
    data = {k: open(v, "rb").read() for k, v in names.items()}
    assert data["none"] == data["pinhole"]
    assert data["lens"] != data["pinhole"] and len(data["lens"]) == len(data["pinhole"])
    assert data["lens75"] != data["lens"]

"""Layered lens records and their filter on the GPU (acn_lens_layers_reduce*, acn_render_lens_layers*, acn_denoise_layers*;
include/actinon_hip.h) against the numpy model of tests/lens_layers_model.py, bit for bit (test_lens_layers_cpu.py checks the model
and that the inputs used here contain what they are there for); the calls' contracts: slices, streams, refusals, the renderer left
alone.  Bit for bit means Y.same_bits: which NaN a NaN result is, the header leaves open."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import lens_layers_model as Y
import lens_surface_model as R
import scenes_util as S
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = dict(aperture=0.15, focus=12.0, jitter=True)
W, H, K = 48, 36, 8
FW, FH = 37, 29


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def flat():
    return A.Scene.build("wine_glass", image_width=W, image_height=H, path_samples=16, direct_samples=50).flatten()


@pytest.fixture(scope="module")
def h(flat):
    """a handle that cuts its lens calls into slices of 1000 rays: 125 positions at K = 8, so the 1728 pixels are 13 slices and 103"""
    mp = pytest.MonkeyPatch()
    mp.setenv("ACN_LENS_SLICE_RAYS", "1000")
    handle = A.Handle(flat)                                                   # (tunables are read at the upload)
    mp.undo()
    yield handle
    handle.close()


def assert_same_bits(got, want):
    bad = Y.same_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def planes(records):
    return np.stack([r.raw for r in records])


# ---- the split against the model ----
@pytest.mark.parametrize("samples", [1, 2, 15, 16, 17, 33, 100])
def test_split_on_synthetic_records(h, detmath_cpu, samples):
    """n on either side of the 16-position tile, K on either side of the 16-sample tile"""
    for n in (1, 15, 16, 17, 33):
        rec, L, _ = Y.synthetic_split(n, samples)
        with np.errstate(all="ignore"):
            want_surf, want_st = Y.split(detmath_cpu, rec, L)
        surf, st = h.lens_layers_reduce(rec, L)
        assert_same_bits(planes(surf), want_surf)
        assert_same_bits(planes(st), want_st)
        assert (planes(st)[:, :, 0].sum(axis=0) == samples).all()
        assert_same_bits(surf[0].raw, h.surface_reduce(rec).raw)              # plane 0 is acn_surface_reduce in all 16 doubles


def test_split_on_a_callers_stream(h, detmath_cpu):
    """device buffers on a torch stream; nothing behind the planes is written, the inputs stay"""
    import torch
    n, samples = 33, 17
    rec, L, _ = Y.synthetic_split(n, samples)
    with np.errstate(all="ignore"):
        want_surf, want_st = Y.split(detmath_cpu, rec, L)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rec, d_L = torch.from_numpy(rec).to("cuda"), torch.from_numpy(L).to("cuda")
        d_surf = torch.full((2 * n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
        d_st = torch.full((3 * n + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
        h.lens_layers_reduce_dev(d_rec.data_ptr(), d_L.data_ptr(), n, samples, d_surf.data_ptr(), d_st.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    surf, st = d_surf.cpu().numpy(), d_st.cpu().numpy()
    assert_same_bits(surf[:2 * n].reshape(2, n, 16), want_surf)
    assert_same_bits(st[:3 * n].reshape(3, n, 8), want_st)
    assert np.isnan(surf[2 * n]).all() and np.isnan(st[3 * n]).all()
    assert_same_bits(d_rec.cpu().numpy(), rec)
    assert_same_bits(d_L.cpu().numpy(), L)


def test_records_do_not_depend_on_neighbours(h):
    rec, L, _ = Y.synthetic_split(33, 33)
    surf, st = h.lens_layers_reduce(rec, L)
    perm = np.random.default_rng(1).permutation(33)
    surf_p, st_p = h.lens_layers_reduce(rec[perm], L[perm])
    assert_same_bits(planes(surf_p), planes(surf)[:, perm])
    assert_same_bits(planes(st_p), planes(st)[:, perm])
    one_surf, one_st = h.lens_layers_reduce(rec[11:12], L[11:12])
    assert_same_bits(planes(one_surf), planes(surf)[:, 11:12])
    assert_same_bits(planes(one_st), planes(st)[:, 11:12])


# ---- end to end on a small scene with an open aperture ----
@pytest.fixture(scope="module")
def layered(h, flat):
    """wine glass 48 x 36 through the open lens, K = 8, jitter: the layered call in uneven slices"""
    pos = S.positions(flat)
    rgb, surf, st = h.render_lens_layers(pos, follow=True, samples=K, seed=0, **LENS)
    out = (pos, rgb, planes(surf), planes(st))
    for a in out:
        a.setflags(write=False)
    return out


def test_layered_call_is_rays_render_surface_split(h, detmath_cpu, layered):
    pos, rgb, surf, st = layered
    lens = dict(LENS, samples=K, seed=0)
    rays = h.lens_rays(pos, **lens)
    rec = h.surface_rays(rays.reshape(-1, 6), follow=True).raw.reshape(len(pos), K, 16)
    L = h.render_rays(rays.reshape(-1, 6), linear=True).reshape(len(pos), K, 3)
    want_surf, want_st = Y.split(detmath_cpu, rec, L)
    assert_same_bits(st, want_st)                                             # all three statistics planes
    assert_same_bits(surf, want_surf)
    assert_same_bits(surf[0], h.surface_lens(pos, follow=True, **lens).raw)   # plane 0 is acn_surface_lens
    assert_same_bits(rgb, h.render_lens(pos, **lens))                         # saturated, as acn_render_lens writes it
    assert (st[:, :, 0].sum(axis=0) == K).all()
    mixed = st[1][:, 0] > 0
    assert mixed.sum() >= 50 and (st[2][:, 0] > 0).any()                      # (an open aperture: edges see two surfaces and more)
    # the split of the device's own records by the reduce call
    r_surf, r_st = h.lens_layers_reduce(rec, L)
    assert_same_bits(planes(r_surf), surf)
    assert_same_bits(planes(r_st), st)


def test_cutting_the_call_by_position_changes_no_bit(h, layered):
    pos, _, surf, st = layered
    lens = dict(LENS, samples=K, seed=0)
    cut = 777
    a = h.render_lens_layers(pos[:cut], follow=True, linear=True, **lens)
    b = h.render_lens_layers(pos[cut:], follow=True, linear=True, **lens)
    assert_same_bits(np.concatenate([planes(a[1]), planes(b[1])], axis=1), surf)
    assert_same_bits(np.concatenate([planes(a[2]), planes(b[2])], axis=1), st)
    assert_same_bits(np.concatenate([a[0], b[0]]), h.render_lens(pos, linear=True, **lens))


def test_main_pass_on_a_callers_stream(h, layered):
    """the main-pass form with a null out_rgb on a torch stream of the caller's against the position form"""
    import torch
    pos, _, surf, st = layered
    first, count = 500, 700
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_surf = torch.full((2 * count + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
        d_st = torch.full((3 * count + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
        h.render_lens_layers_main_pass_dev(first, count, None, d_surf.data_ptr(), d_st.data_ptr(), follow=True, stream=s.cuda_stream,
                                           samples=K, seed=0, **LENS)
    s.synchronize()
    got_surf, got_st = d_surf.cpu().numpy(), d_st.cpu().numpy()
    assert_same_bits(got_surf[:2 * count].reshape(2, count, 16), surf[:, first:first + count])
    assert_same_bits(got_st[:3 * count].reshape(3, count, 8), st[:, first:first + count])
    assert np.isnan(got_surf[2 * count]).all() and np.isnan(got_st[3 * count]).all()


def test_pinhole_identity(h, flat):
    """aperture 0, no jitter, K = 1: plane 0 is acn_render_lens_stats and, in doubles 0 .. 14, acn_surface_positions"""
    pos = S.positions(flat)[::3]
    for follow in (False, True):
        rgb, surf, st = h.render_lens_layers(pos, follow=follow, linear=True, samples=1)
        want_rgb, want_st = h.render_lens_stats(pos, linear=True, samples=1)
        assert_same_bits(st[0].raw, want_st.raw)
        assert_same_bits(rgb, want_rgb)
        assert_same_bits(surf[0].raw[:, :15], h.surface_positions(pos, follow=follow).raw[:, :15])
        assert (surf[0].coverage == 1.0).all() and (surf[1].coverage == 0.0).all()
        assert (st[1].raw == 0).all() and (st[2].raw == 0).all()


# ---- the filter against its model ----
@pytest.fixture(scope="module")
def frame():
    st, rec = Y.synthetic_frame(FW, FH)
    st.setflags(write=False); rec.setflags(write=False)
    return st, rec


@pytest.mark.parametrize("params", [dict(iterations=3), dict(iterations=3, normal_power_log2=2, demodulate=False, sigma_plane=0.3, sigma_lum=2.0)])
def test_filter_against_the_model(h, detmath_cpu, flat, frame, params):
    """37 x 29 is no multiple of the 16-pixel tile; three levels reach stride 4"""
    st, rec = frame
    bg = np.array(flat.params.background_color[:])
    detail = {}
    want = Y.denoise_layers(detmath_cpu, st, rec, FW, FH, bg, detail=detail, **params)
    assert detail["cross"][0] > 0 and detail["cross"][1] > 0                  # minority layers found their neighbours' majority
    got = h.denoise_layers(st, rec, FW, FH, **params)
    assert_same_bits(got, want)


def test_filter_on_a_callers_stream(h, detmath_cpu, flat, frame):
    import torch
    st, rec = frame
    bg = np.array(flat.params.background_color[:])
    want = Y.denoise_layers(detmath_cpu, st, rec, FW, FH, bg, iterations=3)
    n = FW * FH
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_st, d_rec = torch.from_numpy(st.copy()).to("cuda"), torch.from_numpy(rec.copy()).to("cuda")   # (the fixture is read-only)
        d_out = torch.full((n + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
        h.denoise_layers_dev(d_st.data_ptr(), d_rec.data_ptr(), FW, FH, d_out.data_ptr(), stream=s.cuda_stream, iterations=3)
    s.synchronize()
    out = d_out.cpu().numpy()
    assert_same_bits(out[:n].reshape(FH, FW, 3), want)
    assert np.isnan(out[n]).all()
    assert_same_bits(d_st.cpu().numpy(), st)
    assert_same_bits(d_rec.cpu().numpy(), rec)


def test_one_plane_is_denoise_stats(h, frame, layered):
    """with plane 1 and the rest EMPTY the call is acn_denoise_stats( stats plane 0, surface plane 0 ), bit for bit: on the synthetic
    frame and on the rendered one"""
    for st, rec, w, hh in ((frame[0], frame[1], FW, FH), (layered[3], layered[2], W, H)):
        st1 = np.zeros_like(st); st1[0] = st[0]
        rec1 = rec.copy(); rec1[1] = R.miss_record(0, 0.0)
        for params in (dict(iterations=3), dict()):
            assert_same_bits(h.denoise_layers(st1, rec1, w, hh, **params), h.denoise_stats(st[0], rec[0], w, hh, **params))


def test_filter_on_the_rendered_frame(h, detmath_cpu, flat, layered):
    """the records of a render through the model: real edges, real rests"""
    _, _, surf, st = layered
    bg = np.array(flat.params.background_color[:])
    detail = {}
    want = Y.denoise_layers(detmath_cpu, st, surf, W, H, bg, iterations=3, detail=detail)
    assert detail["cross"][1] > 0
    assert_same_bits(h.denoise_layers(st, surf, W, H, iterations=3), want)


def test_the_depth_of_field_tool_with_layers(tmp_path, flat):
    """tools/render_dof.py --layers writes the frame of acn_render_lens_layers -> acn_denoise_layers -> acn_resolve_dev"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_dof as tool
    scene = tmp_path / "scene.npz"
    flat.save(str(scene))
    base = [str(scene), None, "--aperture", "0.15", "--focus", "12", "--samples", "4", "--jitter"]
    data = {}
    for key, extra in (("plain", []), ("layers", ["--layers", "--iterations", "3"])):
        args = list(base)
        args[1] = str(tmp_path / (key + ".pnm"))
        tool.main(args + extra)
        data[key] = open(args[1], "rb").read()
    assert len(data["layers"]) == len(data["plain"]) and data["layers"] != data["plain"]
    hd = A.Handle(flat)
    pos = S.positions(flat)
    _, surf, st = hd.render_lens_layers(pos, follow=True, samples=4, **LENS)
    lin = torch.from_numpy(hd.denoise_layers(st, surf, W, H, iterations=3).reshape(-1, 3)).to("cuda")
    rgb8 = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hd.resolve_dev(lin.data_ptr(), W * H, None, rgb8.data_ptr())
    hd.close()
    assert data["layers"].endswith(rgb8.cpu().numpy().tobytes())


# ---- isolation ----
def test_the_calls_leave_the_renderer_alone(flat, frame):
    pos = S.positions(flat)
    hd = A.Handle(flat)
    hd.render_positions(pos, linear=True)                                   # a warm handle
    before = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    raw = (C.c_double * 25)()
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    raw_before = list(raw)
    counters = hd.last_counters_raw(10)
    kernel_ms = hd.last_kernel_ms()
    rec, L, _ = Y.synthetic_split(33, 33)
    surf, st = hd.lens_layers_reduce(rec, L)
    filtered = hd.denoise_layers(frame[0], frame[1], FW, FH, iterations=3)
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    assert list(raw) == raw_before                                          # [ 23 ], [ 24 ] included: nothing of the workspace moved
    assert list(hd.last_counters_raw(10)) == list(counters) and hd.last_kernel_ms() == kernel_ms
    after = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    assert np.array_equal(before, after)
    # a layered render renders: the frame after it is still the frame before it
    layers = hd.render_lens_layers(pos[::5], follow=True, samples=4, **LENS)
    assert np.array_equal(hd.render_positions(pos, linear=True), before)
    assert_same_bits(planes(hd.render_lens_layers(pos[::5], follow=True, samples=4, **LENS)[2]), planes(layers[2]))
    assert_same_bits(hd.denoise_layers(frame[0], frame[1], FW, FH, iterations=3), filtered)
    assert_same_bits(planes(hd.lens_layers_reduce(rec, L)[1]), planes(st))
    hd.close()


# ---- errors ----
def test_refusals_leave_the_output_untouched(flat, frame):
    """Every ACN_ERR_ARG of the section: the status, acn_last_error, and not one word written, on host and device buffers; then the
    handle still works"""
    import torch
    n, samples = 40, 4
    pos = S.positions(flat)[:n].copy()
    h = A.Handle(flat)
    good = A.Handle.lens_params(samples=samples, aperture=0.1, focus=12.0)
    o = h._plain_opts(False, None)
    rec, L, _ = Y.synthetic_split(n, samples)
    d_pos, d_rec, d_L = torch.from_numpy(pos).to("cuda"), torch.from_numpy(rec).to("cuda"), torch.from_numpy(L).to("cuda")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_surf, d_st, d_rgb = nan(2 * n, 16), nan(3 * n, 8), nan(n, 3)
    surf, st, rgb = np.full((2 * n, 16), np.nan), np.full((3 * n, 8), np.nan), np.full((n, 3), np.nan)
    fst, frec = np.ascontiguousarray(frame[0][:, :n]), np.ascontiguousarray(frame[1][:, :n])   # a frame of 8 x 5 pixels
    d_fst, d_frec = torch.from_numpy(fst).to("cuda"), torch.from_numpy(frec).to("cuda")
    torch.cuda.synchronize()

    def refused(table, word):
        for name, call in table.items():
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert all(np.isnan(a).all() for a in (surf, st, rgb)), name
            assert all(bool(torch.isnan(a).all()) for a in (d_surf, d_st, d_rgb)), name

    def reduce_calls(handle, opts, k=samples, hr=rec.ctypes.data, hl=L.ctypes.data, dr=d_rec.data_ptr(), dl=d_L.data_ptr(), hs=surf.ctypes.data,
                     ht=st.ctypes.data, ds=d_surf.data_ptr(), dt=d_st.data_ptr()):
        return {"reduce": lambda: hip.acn_lens_layers_reduce(handle, hr, hl, n, k, hs, ht, C.byref(opts)),
                "reduce_dev": lambda: hip.acn_lens_layers_reduce_dev(handle, dr, dl, n, k, ds, dt, C.byref(opts))}

    def lens_calls(handle, p, opts, mode=abi.ACN_SURF_FOLLOW, hp=pos.ctypes.data, dp=d_pos.data_ptr(), hs=surf.ctypes.data, ht=st.ctypes.data,
                   ds=d_surf.data_ptr(), dt=d_st.data_ptr(), first=0):
        ref = C.byref(p) if p is not None else None
        return {"layers": lambda: hip.acn_render_lens_layers(handle, hp, n, ref, mode, rgb.ctypes.data, hs, ht, C.byref(opts)),
                "layers_dev": lambda: hip.acn_render_lens_layers_dev(handle, dp, n, ref, mode, d_rgb.data_ptr(), ds, dt, C.byref(opts)),
                "layers_main_pass_dev": lambda: hip.acn_render_lens_layers_main_pass_dev(handle, first, n, ref, mode, d_rgb.data_ptr(), ds, dt, C.byref(opts))}

    def denoise_calls(handle, opts, prm=None, width=8, height=5, hs=fst.ctypes.data, hr=frec.ctypes.data, ds=d_fst.data_ptr(), dr=d_frec.data_ptr(),
                      ho=rgb.ctypes.data, do=d_rgb.data_ptr()):
        ref = C.byref(prm) if prm is not None else None
        return {"denoise": lambda: hip.acn_denoise_layers(handle, hs, hr, width, height, ref, ho, C.byref(opts)),
                "denoise_dev": lambda: hip.acn_denoise_layers_dev(handle, ds, dr, width, height, ref, do, C.byref(opts))}

    only = lambda table, *names: {k: v for k, v in table.items() if k in names}
    # a null handle, or a null buffer with n > 0
    refused(reduce_calls(None, o), "handle")
    refused(lens_calls(None, good, o), "handle")
    refused(denoise_calls(None, o), "null")
    for kw in ("hr", "hl", "hs", "ht"):
        refused(only(reduce_calls(h.h, o, **{kw: None}), "reduce"), "null")
    for kw in ("dr", "dl", "ds", "dt"):
        refused(only(reduce_calls(h.h, o, **{kw: None}), "reduce_dev"), "null")
    refused(only(lens_calls(h.h, good, o, hp=None), "layers"), "null")
    refused(only(lens_calls(h.h, good, o, dp=None), "layers_dev"), "null")
    for kw in ("hs", "ht"):
        refused(only(lens_calls(h.h, good, o, **{kw: None}), "layers"), "null")
    for kw in ("ds", "dt"):
        refused(only(lens_calls(h.h, good, o, **{kw: None}), "layers_dev", "layers_main_pass_dev"), "null")
    for kw in ("hs", "hr", "ho"):
        refused(only(denoise_calls(h.h, o, **{kw: None}), "denoise"), "null")
    for kw in ("ds", "dr", "do"):
        refused(only(denoise_calls(h.h, o, **{kw: None}), "denoise_dev"), "null")
    # K == 0 or K > 4096
    refused(reduce_calls(h.h, o, k=0), "K 0")
    refused(reduce_calls(h.h, o, k=4097), "4097")
    # everything the lens refuses
    small_struct = A.Handle.lens_params(samples=samples, aperture=0.1, focus=12.0)
    small_struct.struct_size = 3
    flags = A.Handle.lens_params(samples=samples, aperture=0.1, focus=12.0)
    flags.flags = 2
    lp = A.Handle.lens_params
    for word, p in (("samples", lp(samples=4097, aperture=0.1, focus=12.0)), ("flags", flags), ("struct_size", small_struct),
                    ("aperture", lp(samples=samples, aperture=-0.1, focus=12.0)), ("aperture", lp(samples=samples, aperture=float("nan"), focus=12.0)),
                    ("focus", lp(samples=samples, aperture=0.1, focus=0.0)), ("focus", lp(samples=samples, aperture=0.1, focus=float("inf")))):
        refused(lens_calls(h.h, p, o), word)
    # an unknown mode; sharding
    refused(lens_calls(h.h, good, o, mode=2), "mode")
    world2 = h._plain_opts(False, None)
    world2.shard_world = 2
    refused(reduce_calls(h.h, world2), "sharded")
    refused(denoise_calls(h.h, world2), "sharded")
    by_samples = h._plain_opts(True, None)
    by_samples.shard_mode, by_samples.shard_rank, by_samples.shard_world = abi.ACN_SHARD_SAMPLES, 0, 2
    refused(lens_calls(h.h, good, by_samples), "ACN_SHARD_SAMPLES")
    unknown = h._plain_opts(False, None)
    unknown.shard_mode = 2
    refused(lens_calls(h.h, good, unknown), "shard_mode")
    # buffers that are not aligned
    refused(only(reduce_calls(h.h, o, dr=d_rec.data_ptr() + 8), "reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, dl=d_L.data_ptr() + 4), "reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, ds=d_surf.data_ptr() + 8), "reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, dt=d_st.data_ptr() + 8), "reduce_dev"), "align")
    refused(only(reduce_calls(h.h, o, hs=surf.ctypes.data + 8), "reduce"), "align")
    refused(only(lens_calls(h.h, good, o, dp=d_pos.data_ptr() + 8), "layers_dev"), "align")
    refused(only(lens_calls(h.h, good, o, ds=d_surf.data_ptr() + 8), "layers_dev", "layers_main_pass_dev"), "align")
    refused(only(lens_calls(h.h, good, o, dt=d_st.data_ptr() + 8), "layers_dev", "layers_main_pass_dev"), "align")
    refused(only(denoise_calls(h.h, o, ds=d_fst.data_ptr() + 8), "denoise_dev"), "align")
    refused(only(denoise_calls(h.h, o, dr=d_frec.data_ptr() + 8), "denoise_dev"), "align")
    # a pixel range outside the image; an open aperture without the scene's focal length
    refused(only(lens_calls(h.h, good, o, first=W * H - n + 1), "layers_main_pass_dev"), "outside")
    nofocal = A.Scene.build("wine_glass", image_width=W, image_height=H, path_samples=16, direct_samples=50, camera_focal_length=0.0).flatten()
    hn = A.Handle(nofocal)
    refused(lens_calls(hn.h, good, o), "focal")
    hn.close()
    # what acn_denoise_stats refuses of a frame and of its parameters
    refused(denoise_calls(h.h, o, width=0), "width")
    refused(denoise_calls(h.h, o, prm=A.Handle.denoise_params(iterations=9)), "iterations")
    refused(denoise_calls(h.h, o, prm=A.Handle.denoise_params(normal_power_log2=11)), "normal_power_log2")
    refused(denoise_calls(h.h, o, prm=A.Handle.denoise_params(sigma_lum=-1.0)), "sigma")
    # n == 0 is ACN_OK and writes nothing, a null buffer included
    for call in (lambda: hip.acn_lens_layers_reduce_dev(h.h, None, None, 0, samples, None, None, C.byref(o)),
                 lambda: hip.acn_lens_layers_reduce(h.h, None, None, 0, 1, surf.ctypes.data, st.ctypes.data, None),
                 lambda: hip.acn_render_lens_layers_dev(h.h, None, 0, C.byref(good), 1, None, None, None, C.byref(o)),
                 lambda: hip.acn_render_lens_layers_main_pass_dev(h.h, 5, 0, C.byref(good), 1, None, d_surf.data_ptr(), d_st.data_ptr(), C.byref(o)),
                 lambda: hip.acn_render_lens_layers(h.h, None, 0, None, 0, None, None, None, None)):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert all(np.isnan(a).all() for a in (surf, st, rgb)) and all(bool(torch.isnan(a).all()) for a in (d_surf, d_st, d_rgb))
    # and the handle works
    got_surf, got_st = h.lens_layers_reduce(rec, L)
    assert (planes(got_st)[:, :, 0].sum(axis=0) == samples).all()
    assert h.denoise_layers(fst, frec, 8, 5, iterations=2).shape == (5, 8, 3)
    h.close()

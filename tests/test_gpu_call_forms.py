"""The frame every entry point of include/actinon_hip.h shares (Call, DevCopies and pixel_range_check in csrc/acn_handle.h), on the
64 x 36 wine glass of smoke().

1. The pixel range of acn_render_main_pass_dev and acn_render_main_pass_shard_dev is refused when first + count wraps or ends behind
   the image: ACN_ERR_ARG, "pixel range outside the image", nothing launched and nothing written, and the handle renders the whole
   frame to the bits it gave before.
2. A host-buffer form gives the bits of its device-buffer form, at sizes that are no round number.  acn_select_above and
   acn_key_histogram are left to test_gpu_select.py::test_a_callers_stream_and_the_host_form, which holds both forms of both calls
   against one model at n = one tile + 1 already.
3. The lens calls share one slice loop (lens_slices in csrc/acn_calls.hip): cut into slices of 13, 13 and 11 positions, or of one
   position each, every family gives the bits of the uncut call, and the families agree where their contracts say they do."""
import ctypes as C

import numpy as np
import pytest

import actinon_amd as A
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
W, H = 64, 36
PIXELS = W * H
N = 37                                      # positions or rays of a pair: no stride hides behind a round number
LENS = dict(samples=3, aperture=0.15, focus=12.0, jitter=True, seed=5)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def flat():
    return A.Scene.build("wine_glass", image_width=W, image_height=H, path_samples=16, direct_samples=50).flatten()


@pytest.fixture(scope="module")
def h(flat):
    handle = A.Handle(flat)
    yield handle
    handle.close()


@pytest.fixture(scope="module")
def pos():
    """37 positions spread over the raster, off the pixel centres"""
    rng = np.random.default_rng(37)
    return np.stack([rng.random(N) * W, rng.random(N) * H], axis=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def on_device(torch, h, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(torch.device("cuda", h.device))


def empty(torch, h, *shape):
    return torch.full(shape, -7.25, dtype=torch.float64, device=torch.device("cuda", h.device))


def test_a_pixel_range_that_wraps_or_overhangs_is_refused(h, torch):
    dev = torch.device("cuda", h.device)
    whole = empty(torch, h, PIXELS, 3)
    h.render_main_pass_dev(0, PIXELS, whole.data_ptr(), linear=True)
    before = whole.cpu().numpy().copy()
    o = h._opts(True, None)
    padded = hip.acn_shard_tile_padded(PIXELS, 2)
    for first, count in ((2 ** 64 - 4, 8), (PIXELS - 10, 11)):
        out = empty(torch, h, max(PIXELS, 2 * padded), 3)
        torch.cuda.synchronize(dev)
        calls = {"acn_render_main_pass_dev": lambda: hip.acn_render_main_pass_dev(h.h, first, count, out.data_ptr(), C.byref(o)),
                 "acn_render_main_pass_shard_dev": lambda: hip.acn_render_main_pass_shard_dev(h.h, first, count, 1, 2, out.data_ptr(), C.byref(o))}
        for name, call in calls.items():
            assert call() == abi.ACN_ERR_ARG, (name, first, count)
            assert b"pixel range outside the image" in hip.acn_last_error(), (name, hip.acn_last_error())
        torch.cuda.synchronize(dev)
        assert bool((out == -7.25).all()), (first, count)
    h.render_main_pass_dev(0, PIXELS, whole.data_ptr(), linear=True)
    assert same_bits(whole.cpu().numpy(), before)
    # the last pixels alone are a range inside the image: the bits of the frame's
    tail = empty(torch, h, 10, 3)
    h.render_main_pass_dev(PIXELS - 10, 10, tail.data_ptr(), linear=True)
    assert same_bits(tail.cpu().numpy(), before[PIXELS - 10:])


def test_render_forms(h, torch, pos):
    """render_positions, camera_rays, render_rays: host form against device form"""
    d_pos = on_device(torch, h, pos)
    d_rgb, d_rays = empty(torch, h, N, 3), empty(torch, h, N, 6)
    for linear in (True, False):
        h.render_positions_dev(d_pos.data_ptr(), N, d_rgb.data_ptr(), linear=linear)
        assert same_bits(h.render_positions(pos, linear=linear), d_rgb.cpu().numpy()), linear
    h.camera_rays_dev(d_pos.data_ptr(), N, d_rays.data_ptr())
    rays = h.camera_rays(pos)
    assert same_bits(rays, d_rays.cpu().numpy())
    for linear in (True, False):
        h.render_rays_dev(d_rays.data_ptr(), N, d_rgb.data_ptr(), linear=linear)
        assert same_bits(h.render_rays(rays, linear=linear), d_rgb.cpu().numpy()), linear


def test_surface_forms(h, torch, pos):
    rays = h.camera_rays(pos)
    d_pos, d_rays = on_device(torch, h, pos), on_device(torch, h, rays)
    for follow in (False, True):
        d_rec = empty(torch, h, N, abi.ACN_SURF_STRIDE)
        h.surface_positions_dev(d_pos.data_ptr(), N, d_rec.data_ptr(), follow=follow)
        assert same_bits(h.surface_positions(pos, follow=follow).raw, d_rec.cpu().numpy()), follow
        d_rec.fill_(-7.25)
        h.surface_rays_dev(d_rays.data_ptr(), N, d_rec.data_ptr(), follow=follow)
        assert same_bits(h.surface_rays(rays, follow=follow).raw, d_rec.cpu().numpy()), follow


def test_denoise_forms_on_a_9_by_5_frame(h, torch):
    w, hh = 9, 5
    frame_pos = A.main_pass_positions(W, H).reshape(H, W, 2)[7:7 + hh, 20:20 + w].reshape(-1, 2)     # across the glass
    lin = h.render_positions(frame_pos, linear=True).reshape(hh, w, 3)
    rec = h.surface_positions(frame_pos, follow=True).raw
    stats = h.render_lens_stats(frame_pos, linear=True, samples=4, jitter=True)[1].raw
    d_lin, d_rec, d_stats = on_device(torch, h, lin), on_device(torch, h, rec), on_device(torch, h, stats)
    d_out = empty(torch, h, hh * w, 3)
    h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr(), w, hh, d_out.data_ptr(), iterations=3)
    host = h.denoise(lin, rec, iterations=3)
    assert same_bits(host.reshape(-1, 3), d_out.cpu().numpy())
    h.denoise_dev(d_lin.data_ptr(), d_rec.data_ptr(), w, hh, d_lin.data_ptr(), iterations=3)      # in place, as the host form works
    assert same_bits(host.reshape(-1, 3), d_lin.cpu().numpy().reshape(-1, 3))
    d_out.fill_(-7.25)
    h.denoise_stats_dev(d_stats.data_ptr(), d_rec.data_ptr(), w, hh, d_out.data_ptr(), iterations=3)
    assert same_bits(h.denoise_stats(stats, rec, w, hh, iterations=3).reshape(-1, 3), d_out.cpu().numpy())


def test_lens_forms(h, torch, pos):
    K = LENS["samples"]
    d_pos = on_device(torch, h, pos)
    d_rays = empty(torch, h, N, K, 6)
    h.lens_rays_dev(d_pos.data_ptr(), N, d_rays.data_ptr(), **LENS)
    assert same_bits(h.lens_rays(pos, **LENS), d_rays.cpu().numpy())
    d_two = empty(torch, h, N, 2, 6)
    h.lens_rays_dev(d_pos.data_ptr(), N, d_two.data_ptr(), first_sample=1, n_samples=2, **LENS)
    assert same_bits(h.lens_rays(pos, first_sample=1, n_samples=2, **LENS), d_two.cpu().numpy())
    d_rgb, d_st = empty(torch, h, N, 3), empty(torch, h, N, abi.ACN_STATS_STRIDE)
    for linear in (True, False):
        h.render_lens_dev(d_pos.data_ptr(), N, d_rgb.data_ptr(), linear=linear, **LENS)
        assert same_bits(h.render_lens(pos, linear=linear, **LENS), d_rgb.cpu().numpy()), linear
        d_rgb.fill_(-7.25)
        h.render_lens_stats_dev(d_pos.data_ptr(), N, d_rgb.data_ptr(), d_st.data_ptr(), linear=linear, **LENS)
        rgb, st = h.render_lens_stats(pos, linear=linear, **LENS)
        assert same_bits(rgb, d_rgb.cpu().numpy()) and same_bits(st.raw, d_st.cpu().numpy()), linear
    # out_rgb = NULL in both forms: the records alone, the same ones
    want = d_st.cpu().numpy()
    d_st.fill_(-7.25)
    h.render_lens_stats_dev(d_pos.data_ptr(), N, None, d_st.data_ptr(), **LENS)
    raw = np.full((N, abi.ACN_STATS_STRIDE), -7.25)
    p, o = h.lens_params(**LENS), h._opts(False, None)
    A.check(hip.acn_render_lens_stats(h.h, pos.ctypes.data, N, C.byref(p), None, raw.ctypes.data, C.byref(o)), "acn_render_lens_stats")
    assert same_bits(raw, d_st.cpu().numpy()) and same_bits(raw, want)


def test_merge_forms_with_an_index(h, torch, pos):
    """n_part = 5 records into n_acc = 37, through an index"""
    acc = h.render_lens_stats(pos, samples=4, seed=3, jitter=True)[1].raw
    idx = np.array([36, 0, 17, 5, 21], dtype=np.int64)
    part = h.render_lens_stats(pos[idx], samples=2, seed=4, jitter=True)[1].raw
    d_acc, d_part, d_idx = on_device(torch, h, acc), on_device(torch, h, part), on_device(torch, h, idx)
    h.lens_stats_merge_dev(d_acc.data_ptr(), N, d_part.data_ptr(), 5, d_idx.data_ptr())
    got = h.lens_stats_merge(acc, part, index=idx).raw
    assert same_bits(got, d_acc.cpu().numpy())
    rest = np.setdiff1d(np.arange(N), idx)
    assert same_bits(got[rest], acc[rest]) and (got[idx, 0] == 6).all()     # five records took two samples more, the others none


def planes(records):
    return np.stack([r.raw for r in records])


def test_lens_record_forms(h, torch, pos):
    """surface_reduce, surface_lens, lens_layers_reduce, render_lens_layers: host form against device form"""
    K = LENS["samples"]
    rays = h.lens_rays(pos, **LENS).reshape(-1, 6)
    rec = h.surface_rays(rays, follow=True).raw.reshape(N, K, abi.ACN_SURF_STRIDE)
    rad = h.render_rays(rays, linear=True).reshape(N, K, 3)
    d_pos, d_rec, d_rad = on_device(torch, h, pos), on_device(torch, h, rec), on_device(torch, h, rad)
    d_one = empty(torch, h, N, abi.ACN_SURF_STRIDE)
    h.surface_reduce_dev(d_rec.data_ptr(), N, K, d_one.data_ptr())
    assert same_bits(h.surface_reduce(rec).raw, d_one.cpu().numpy())
    for follow in (False, True):
        d_one.fill_(-7.25)
        h.surface_lens_dev(d_pos.data_ptr(), N, d_one.data_ptr(), follow=follow, **LENS)
        assert same_bits(h.surface_lens(pos, follow=follow, **LENS).raw, d_one.cpu().numpy()), follow
    d_rgb = empty(torch, h, N, 3)
    d_surf = empty(torch, h, abi.ACN_LAYERS_SURFACE_PLANES, N, abi.ACN_SURF_STRIDE)
    d_st = empty(torch, h, abi.ACN_LAYERS_STATS_PLANES, N, abi.ACN_STATS_STRIDE)
    h.lens_layers_reduce_dev(d_rec.data_ptr(), d_rad.data_ptr(), N, K, d_surf.data_ptr(), d_st.data_ptr())
    surf, st = h.lens_layers_reduce(rec, rad)
    assert same_bits(planes(surf), d_surf.cpu().numpy()) and same_bits(planes(st), d_st.cpu().numpy())
    d_surf.fill_(-7.25), d_st.fill_(-7.25)
    h.render_lens_layers_dev(d_pos.data_ptr(), N, d_rgb.data_ptr(), d_surf.data_ptr(), d_st.data_ptr(), follow=True, **LENS)
    rgb, surf, st = h.render_lens_layers(pos, follow=True, **LENS)
    want_surf, want_st = d_surf.cpu().numpy(), d_st.cpu().numpy()
    assert same_bits(rgb, d_rgb.cpu().numpy()) and same_bits(planes(surf), want_surf) and same_bits(planes(st), want_st)
    # out_rgb = NULL in both forms: the planes alone, the same ones
    d_surf.fill_(-7.25), d_st.fill_(-7.25)
    h.render_lens_layers_dev(d_pos.data_ptr(), N, None, d_surf.data_ptr(), d_st.data_ptr(), follow=True, **LENS)
    raw_surf, raw_st = np.full(want_surf.shape, -7.25), np.full(want_st.shape, -7.25)
    p, o = h.lens_params(**LENS), h._opts(False, None)
    A.check(hip.acn_render_lens_layers(h.h, pos.ctypes.data, N, C.byref(p), abi.ACN_SURF_FOLLOW, None, raw_surf.ctypes.data, raw_st.ctypes.data,
                                       C.byref(o)), "acn_render_lens_layers")
    assert same_bits(raw_surf, d_surf.cpu().numpy()) and same_bits(raw_st, d_st.cpu().numpy())
    assert same_bits(raw_surf, want_surf) and same_bits(raw_st, want_st)


def test_denoise_layers_forms_on_a_9_by_5_frame(h, torch):
    w, hh = 9, 5
    frame_pos = A.main_pass_positions(W, H).reshape(H, W, 2)[7:7 + hh, 20:20 + w].reshape(-1, 2)     # across the glass
    _, surf, st = h.render_lens_layers(frame_pos, follow=True, linear=True, samples=4, jitter=True)
    d_surf, d_st = on_device(torch, h, planes(surf)), on_device(torch, h, planes(st))
    d_out = empty(torch, h, hh * w, 3)
    h.denoise_layers_dev(d_st.data_ptr(), d_surf.data_ptr(), w, hh, d_out.data_ptr(), iterations=3)
    assert same_bits(h.denoise_layers(st, surf, w, hh, iterations=3).reshape(-1, 3), d_out.cpu().numpy())


def same_bits_or_nan(a, b):
    """bit for bit, and a NaN matches a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def lens_families(handle, pos):
    """the four families that cut their positions into slices, on one handle"""
    rgb = handle.render_lens(pos, linear=True, **LENS)
    stats_rgb, stats = handle.render_lens_stats(pos, linear=True, **LENS)
    surface = handle.surface_lens(pos, follow=True, **LENS).raw
    layers_rgb, layers_surf, layers_st = handle.render_lens_layers(pos, follow=True, linear=True, **LENS)
    return {"render_lens": rgb, "render_lens_stats rgb": stats_rgb, "render_lens_stats": stats.raw, "surface_lens": surface,
            "render_lens_layers rgb": layers_rgb, "render_lens_layers surface": planes(layers_surf), "render_lens_layers stats": planes(layers_st)}


@pytest.fixture(scope="module")
def uncut(h, pos):
    """the families at the default slice size: the 37 positions are one slice"""
    return lens_families(h, pos)


@pytest.mark.parametrize("slice_rays", [40, 2])
def test_all_lens_families_cut_alike(flat, pos, uncut, slice_rays):
    """K = 3: 40 rays are slices of 13, 13 and 11 of the 37 positions; 2 rays are less than one position's, so every slice is one"""
    mp = pytest.MonkeyPatch()
    mp.setenv("ACN_LENS_SLICE_RAYS", str(slice_rays))
    cut = A.Handle(flat)                                                      # (tunables are read at the upload)
    mp.undo()
    try:
        got = lens_families(cut, pos)
    finally:
        cut.close()
    for name, want in uncut.items():
        assert same_bits_or_nan(got[name], want), (slice_rays, name)
    assert same_bits_or_nan(got["render_lens_layers surface"][0], got["surface_lens"]), slice_rays
    assert same_bits_or_nan(got["render_lens_layers rgb"], got["render_lens"]), slice_rays

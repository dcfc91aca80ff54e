"""The thin-lens camera on the GPU (acn_lens_rays, acn_render_lens*; include/actinon_hip.h): the ray generator against the numpy
model of tests/lens_model.py bit for bit, the render call against the library's own position and ray calls bit for bit, and
against the CPU oracle ray by ray through the pinhole-of-a-ray construction of tests/test_gpu_rays.py."""
import ctypes as C

import numpy as np
import pytest

import actinon_amd as A
import lens_model as M
import scenes_util as S
from actinon_amd import abi
from actinon_amd._lib import hip
from test_gpu_rays import pinhole_of_ray

pytestmark = pytest.mark.gpu
TOL = 1e-9          # the project's bound for GPU <-> oracle


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def small(name, n):
    """scene `name` of scenes_util.SMALL and about n of its pixel centres, spread over the raster"""
    sc, flat = S.build(name)
    pos = S.positions(flat)
    return flat, pos[:: max(1, len(pos) // n)][:n].copy()


@pytest.mark.parametrize("width,height", [(7, 5), (24, 16)])
def test_lens_rays_equal_the_model(detmath_cpu, oracle, width, height):
    """acn_lens_rays is the generator the header states: every ray of every sample equals tests/lens_model.py bit for bit --
    with and without jitter, closed and open aperture, two seeds, a window of samples, one position, and through the device
    entry point on a torch stream of the caller's."""
    import torch
    flat = A.Scene.build("wine_glass", image_width=width, image_height=height, path_samples=4, direct_samples=4).flatten()
    pos = S.positions(flat)
    n, K = len(pos), 5
    h = A.Handle(flat)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pos = torch.from_numpy(pos).to("cuda")
        d_rays = torch.empty((n, K, 6), dtype=torch.float64, device="cuda")
    for jitter in (False, True):
        for aperture, focus in ((0.0, 0.0), (0.35, 11.0)):
            for seed in (0, 77):
                kw = dict(samples=K, aperture=aperture, focus=focus, jitter=jitter, seed=seed)
                want = M.lens_rays(detmath_cpu, oracle, flat.params, pos, **kw)
                got = h.lens_rays(pos, **kw)
                assert got.shape == (n, K, 6)
                assert np.array_equal(got, want), (jitter, aperture, seed, np.argwhere(got != want)[:4])
                with torch.cuda.stream(s):
                    d_rays.fill_(float("nan"))
                    h.lens_rays_dev(d_pos.data_ptr(), n, d_rays.data_ptr(), stream=s.cuda_stream, **kw)
                s.synchronize()
                assert np.array_equal(d_rays.cpu().numpy(), want), (jitter, aperture, seed)
    kw = dict(samples=K, aperture=0.35, focus=11.0, jitter=True, seed=77)
    full = h.lens_rays(pos, **kw)
    assert np.array_equal(h.lens_rays(pos, first_sample=2, n_samples=2, **kw), full[:, 2:4])
    assert np.array_equal(h.lens_rays(pos[3:4], **kw), full[3:4])                       # n = 1
    assert np.array_equal(h.lens_rays(pos[3:4], first_sample=4, n_samples=1, **kw), full[3:4, 4:5])
    # a closed aperture without jitter: the pipeline's own camera rays, K times
    assert np.array_equal(h.lens_rays(pos, samples=K), np.repeat(h.camera_rays(pos)[:, None, :], K, axis=1))
    # the default K
    assert h.lens_rays(pos[:2]).shape == (2, abi.ACN_LENS_DEFAULT_SAMPLES, 6)
    h.close()


@pytest.mark.parametrize("name", ["wine_glass_c2", "primitives_path"])
def test_pinhole_identities(name):
    """K = 1 without jitter and with a closed aperture is acn_render_positions; K = 3 is ( ( ( 0 + L ) + L ) + L ) / 3 of the
    linear position render, and its saturated form is cl_s_sat of that.  All bit for bit."""
    import torch
    flat, pos = small(name, 80)
    h = A.Handle(flat)
    lin = h.render_positions(pos, linear=True)
    sat = h.render_positions(pos, linear=False)
    assert np.array_equal(h.render_lens(pos, linear=True, samples=1), lin)
    assert np.array_equal(h.render_lens(pos, linear=False, samples=1), sat)
    mean3 = (((0.0 + lin) + lin) + lin) / 3.0
    assert np.array_equal(h.render_lens(pos, linear=True, samples=3), mean3)
    d = torch.from_numpy(mean3).to("cuda")
    h.resolve_dev(d.data_ptr(), len(pos), d.data_ptr(), None)
    assert np.array_equal(h.render_lens(pos, linear=False, samples=3), d.cpu().numpy())
    h.close()


LENS = dict(samples=4, aperture=0.15, focus=12.0, jitter=True, seed=3)


@pytest.mark.parametrize("lanes", [None, "1"])
def test_render_lens_is_the_ordered_mean_of_its_rays(monkeypatch, lanes):
    """acn_render_lens = acn_lens_rays -> acn_render_rays (linear) -> the mean in the order of k ( -> cl_s_sat ), bit for bit:
    in three slices, the last one short (600 positions, K = 4, 1024 rays per slice), and in one; the main-pass form equals
    the position form on the same pixel centres; a whole raster on the concurrent lanes."""
    import torch
    if lanes:
        monkeypatch.setenv("ACN_LANES", lanes)
    else:
        monkeypatch.delenv("ACN_LANES", raising=False)
    sc, flat = S.build("wine_glass_c2")
    allpos = S.positions(flat)
    pos = allpos[::8][:600].copy()
    n, K = len(pos), LENS["samples"]
    assert n == 600
    monkeypatch.setenv("ACN_LENS_SLICE_RAYS", "1024")
    h = A.Handle(flat)                                                      # (tunables are read at the upload)
    monkeypatch.delenv("ACN_LENS_SLICE_RAYS")
    one = A.Handle(flat)
    rays = h.lens_rays(pos, **LENS)
    L = h.render_rays(rays.reshape(n * K, 6), linear=True).reshape(n, K, 3)
    mean = M.ordered_mean(L)
    got = h.render_lens(pos, linear=True, **LENS)
    assert np.array_equal(got, mean), np.argwhere(got != mean)[:4]
    assert np.array_equal(one.render_lens(pos, linear=True, **LENS), mean)
    d = torch.from_numpy(mean).to("cuda")
    h.resolve_dev(d.data_ptr(), n, d.data_ptr(), None)
    assert np.array_equal(h.render_lens(pos, linear=False, **LENS), d.cpu().numpy())
    assert np.array_equal(one.render_lens(pos, linear=False, **LENS), d.cpu().numpy())
    # pixel centres [ first, first + count ): generated on the device or handed in, on a stream of the caller's
    first, count = 1000, 700
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_pos = torch.from_numpy(allpos[first:first + count]).to("cuda")
        a = torch.full((count, 3), float("nan"), dtype=torch.float64, device="cuda")
        b = torch.full((count, 3), float("nan"), dtype=torch.float64, device="cuda")
        for linear in (True, False):
            h.render_lens_main_pass_dev(first, count, a.data_ptr(), linear=linear, stream=s.cuda_stream, **LENS)
            h.render_lens_dev(d_pos.data_ptr(), count, b.data_ptr(), linear=linear, stream=s.cuda_stream, **LENS)
            s.synchronize()
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), linear
    assert np.array_equal(a.cpu().numpy(), h.render_lens(allpos[first:first + count], **LENS))
    # the whole raster at K = 8: 41 472 rays in one slice, enough for two lanes where lanes are allowed
    big = dict(LENS, samples=8)
    nb = len(allpos)
    c = torch.empty((nb, 3), dtype=torch.float64, device="cuda")
    one.render_lens_main_pass_dev(0, nb, c.data_ptr(), linear=True, **big)
    rb = one.lens_rays(allpos, **big)
    Lb = one.render_rays(rb.reshape(nb * 8, 6), linear=True).reshape(nb, 8, 3)
    assert np.array_equal(c.cpu().numpy(), M.ordered_mean(Lb))
    h.close()
    one.close()


ORACLE_POS = np.array([[44.5, 11.5], [46.5, 14.5], [47.5, 21.5], [52.5, 31.5], [48.5, 26.5],         # the glass
                       [47.5, 17.5],                                                                   # the wine
                       [10.5, 40.5], [80.5, 20.5], [30.5, 50.5],                                       # the table
                       [48.5, -60.5], [10.5, -80.5], [90.5, -55.5]])                                   # above the raster: sky


def test_lens_against_the_oracle(oracle):
    """Every lens ray rendered by the CPU oracle as the central ray of a pinhole of its own; the mean in the order of k
    against the device."""
    sc, flat = S.build("wine_glass_c2")
    sc2, cpu_flat = S.build("wine_glass_c2")                               # (pinhole_of_ray rewrites its camera)
    kw = dict(samples=4, aperture=0.15, focus=12.0, jitter=True)
    n, K = len(ORACLE_POS), 4
    h = A.Handle(flat)
    rays = h.lens_rays(ORACLE_POS, **kw).reshape(n * K, 6)
    d = rays[:, 3:]
    assert (d != 0).all() and (np.abs((d * d).sum(axis=1) - 1.0) < 1e-8).all()
    surf = h.surface_rays(rays)
    assert (~surf.hit).sum() >= 1, "no lens ray misses"
    assert (surf.hit & ((surf.kind & abi.ACN_SURF_TRANSPARENT) != 0)).sum() >= 1, "no lens ray enters glass"
    gpu = h.render_lens(ORACLE_POS, linear=True, **kw)
    h.close()
    cpu = np.empty((n * K, 3))
    for i in range(n * K):
        cpu[i] = oracle.render_positions(cpu_flat, pinhole_of_ray(cpu_flat, rays[i, :3], rays[i, 3:]), linear=True, threads=1)[0]
    bg = np.array(flat.params.background_color[:])
    assert (np.abs(cpu - bg).max(axis=1) == 0).sum() >= 1                  # a miss returns the background
    err = np.abs(gpu - M.ordered_mean(cpu.reshape(n, K, 3))).max(axis=1)
    print("max |gpu - oracle| per position:", err)
    assert err.max() <= TOL, (np.flatnonzero(err > TOL), err.max())


def test_it_focuses(detmath_cpu):
    """The plane in focus is where the lens rays of a pixel meet: on a diffuse surface at the focus distance all K rays hit
    the point the pinhole ray hits; on a surface whose view depth differs by more than 20 % they spread."""
    sc, flat = S.build("primitives_c1")
    prm = flat.params
    w, hh = int(prm.image_width), int(prm.image_height)
    pos = S.positions(flat)
    cam = M.Camera(detmath_cpu, prm)
    h = A.Handle(flat)
    s = h.surface_positions(pos)
    depth = ((s.position - cam.position) * cam.V).sum(axis=1)
    plain = s.hit & ((s.kind & abi.ACN_SURF_DIFFUSE) != 0) & ((s.kind & (abi.ACN_SURF_EMITTER | abi.ACN_SURF_TRANSPARENT)) == 0)
    # a pixel whose 9 x 9 neighbourhood shows the same object (the lens rays must not slip past its edge)
    obj = np.where(plain, s.enter, -2).reshape(hh, w)
    same = np.ones((hh, w), dtype=bool)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            same &= np.roll(np.roll(obj, dy, axis=0), dx, axis=1) == obj
    same[:4] = same[-4:] = False
    same[:, :4] = same[:, -4:] = False
    same = same.reshape(-1) & plain
    # of those the pixel that faces the camera most.  A reported hit lies a little short of the surface along its ray (about 1e-6
    # on these objects), so rays that meet in P at angles up to aperture / focus apart report points that far apart times the
    # angle, more at grazing incidence: 1e-6 * 0.002 / 10 is well inside 1e-9 * |P|, which aperture 0.05 or a floor pixel is not
    facing = np.abs((h.camera_rays(pos)[:, 3:] * s.exit_normal).sum(axis=1))
    cand = np.flatnonzero(same)
    assert len(cand) > 0
    i = cand[np.argmax(facing[cand])]
    P, focus, aperture, K = s.position[i], depth[i], 0.002, 8
    assert facing[i] > 0.99
    assert focus > 0
    kw = dict(samples=K, aperture=aperture, focus=focus)
    r = h.surface_rays(h.lens_rays(pos[i:i + 1], **kw).reshape(K, 6))
    assert r.hit.all() and (r.enter == s.enter[i]).all(), (r.enter, s.enter[i])
    off = np.sqrt(((r.position - P) ** 2).sum(axis=1))
    print("in focus: |hit - P| =", off, "of |P| =", np.sqrt(P @ P))
    assert off.max() <= 1e-9 * np.sqrt(P @ P)
    # a second pixel, at another depth
    far = np.flatnonzero(same & (np.abs(depth / focus - 1.0) > 0.2))
    assert len(far) > 0
    j = far[len(far) // 2]
    assert abs(depth[j] / focus - 1.0) > 0.2
    r2 = h.surface_rays(h.lens_rays(pos[j:j + 1], **kw).reshape(K, 6))
    assert r2.hit.all()
    spread = np.sqrt(((r2.position[:, None, :] - r2.position[None, :, :]) ** 2).sum(axis=-1)).max()
    print("out of focus: depth", depth[j], "focus", focus, "spread", spread)
    assert spread > 1e-3 * aperture
    h.close()


def lens_struct(**kw):
    return A.Handle.lens_params(**kw)


def test_refusals_leave_the_output_untouched():
    """Every ACN_ERR_ARG of the header: the status, acn_last_error, and not one word written -- on host and device buffers, for
    the ray and the render calls.  Then the cancel flag, and the handle still renders."""
    import torch
    flat, pos = small("wine_glass_c2", 40)
    n, K = len(pos), 4
    h = A.Handle(flat)
    sc0 = A.Scene.build("wine_glass", image_width=96, image_height=54, path_samples=4, direct_samples=4, camera_focal_length=0.0)
    h0 = A.Handle(sc0.flatten())                                            # a camera without a focal length
    good = dict(samples=K, aperture=0.1, focus=12.0)
    o = h._opts(True, None)
    d_pos = torch.from_numpy(pos).to("cuda")
    d_out = torch.full((n, K, 6), float("nan"), dtype=torch.float64, device="cuda")
    out = np.full((n, K, 6), np.nan)

    def calls(handle, p, first_sample=0, n_samples=K, hp=pos.ctypes.data, ho=None, do=None):
        """the five entry points with parameters p; the ray calls with the given window.  hp: host positions; ho, do: host and
        device output (0: a null pointer)"""
        ho = out.ctypes.data if ho is None else ho
        do = d_out.data_ptr() if do is None else do
        dp = d_pos.data_ptr()
        ref = C.byref(p)
        return {"lens_rays": lambda: hip.acn_lens_rays(handle, hp, n, ref, first_sample, n_samples, ho),
                "lens_rays_dev": lambda: hip.acn_lens_rays_dev(handle, dp, n, ref, first_sample, n_samples, do, C.byref(o)),
                "render_lens": lambda: hip.acn_render_lens(handle, hp, n, ref, ho, C.byref(o)),
                "render_lens_dev": lambda: hip.acn_render_lens_dev(handle, dp, n, ref, do, C.byref(o)),
                "render_lens_main_pass_dev": lambda: hip.acn_render_lens_main_pass_dev(handle, 0, n, ref, do, C.byref(o))}

    def refused(table, only=None, word=None):
        for name, call in table.items():
            if only and name not in only:
                continue
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and (word or "") in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(out).all() and bool(torch.isnan(d_out).all()), name

    small_struct = lens_struct(**good)
    small_struct.struct_size = 3
    cases = [("samples", lens_struct(samples=4097, aperture=0.1, focus=12.0)),
             ("flags", lens_struct(**good)), ("struct_size", small_struct),
             ("aperture", lens_struct(samples=K, aperture=-0.1, focus=12.0)),
             ("aperture", lens_struct(samples=K, aperture=float("nan"), focus=12.0)),
             ("aperture", lens_struct(samples=K, aperture=float("inf"), focus=12.0)),
             ("focus", lens_struct(samples=K, aperture=0.1, focus=0.0)),
             ("focus", lens_struct(samples=K, aperture=0.1, focus=-3.0)),
             ("focus", lens_struct(samples=K, aperture=0.1, focus=float("inf"))),
             ("focus", lens_struct(samples=K, aperture=0.1, focus=float("nan")))]
    cases[1][1].flags = 2
    for word, p in cases:
        refused(calls(h.h, p), word=word)
    refused(calls(h0.h, lens_struct(**good)), word="focal")
    refused(calls(None, lens_struct(**good)), word="null")
    good_p = lens_struct(**good)
    refused(calls(h.h, good_p, hp=None), only=("lens_rays", "render_lens"), word="null")
    refused(calls(h.h, good_p, ho=0, do=0), word="null")
    refused({"lens_rays_dev": lambda: hip.acn_lens_rays_dev(h.h, None, n, C.byref(good_p), 0, K, d_out.data_ptr(), C.byref(o)),
             "render_lens_dev": lambda: hip.acn_render_lens_dev(h.h, None, n, C.byref(good_p), d_out.data_ptr(), C.byref(o))}, word="null")
    # the window of a ray call
    for first_sample, n_samples in ((0, 0), (K, 1), (1, K), (0, K + 1), (0xFFFFFFFF, 2)):
        refused(calls(h.h, good_p, first_sample, n_samples), only=("lens_rays", "lens_rays_dev"), word="sample")
    # a pixel range outside the raster; samples sharded without linear output
    outside = {"main": lambda: hip.acn_render_lens_main_pass_dev(h.h, 96 * 54 - 10, 11, C.byref(good_p), d_out.data_ptr(), C.byref(o))}
    refused(outside, word="outside")
    o.flags = 0
    o.shard_mode, o.shard_rank, o.shard_world = abi.ACN_SHARD_SAMPLES, 0, 2
    refused(calls(h.h, good_p), only=("render_lens", "render_lens_dev", "render_lens_main_pass_dev"), word="LINEAR")
    # a closed aperture reads no focus distance, and a camera without a focal length may use it
    o = h._opts(True, None)
    assert hip.acn_lens_rays(h0.h, pos.ctypes.data, n, C.byref(lens_struct(samples=K, focus=float("nan"))), 0, K, out.ctypes.data) == abi.ACN_OK
    assert np.isfinite(out[..., :3]).all()
    # cancelled before it starts; then the handle renders as before
    want = h.render_lens(pos, linear=True, **good)
    h.cancel = C.c_int(1)
    with pytest.raises(A.AcnError) as e:
        h.render_lens(pos, linear=True, **good)
    assert e.value.status == abi.ACN_ERR_CANCELLED
    h.cancel = None
    assert np.array_equal(h.render_lens(pos, linear=True, **good), want)
    h.close()
    h0.close()


def test_good_neighbour():
    """A lens call leaves nothing behind: position renders before and after it are the same bits and no call redoes a chunk;
    the same for a denoise call, whose scratch memory is apart from the lens buffers."""
    sc, flat = S.build("wine_glass_c2")
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    pos = S.positions(flat)
    h = A.Handle(flat)
    h.render_positions(pos, linear=True)                                    # a warm handle
    before = h.render_positions(pos, linear=True)
    assert h.last_stages()["retries"] == 0
    surf = h.surface_positions(pos, follow=True)
    den = h.denoise(before.reshape(hh, w, 3), surf, iterations=3)
    lens = h.render_lens(pos, linear=True, **LENS)
    assert h.last_stages()["retries"] == 0
    assert np.isfinite(lens).all()
    after = h.render_positions(pos, linear=True)
    assert h.last_stages()["retries"] == 0
    assert np.array_equal(before, after)
    assert np.array_equal(h.denoise(after.reshape(hh, w, 3), surf, iterations=3), den)
    assert np.array_equal(h.render_lens(pos, linear=True, **LENS), lens)
    # sample shards: the partial means add up to the mean
    total = np.zeros_like(lens)
    for rank in range(2):
        h.sample_shard = (rank, 2)
        total += h.render_lens(pos, linear=True, **LENS)
    h.sample_shard = None
    assert np.abs(total - lens).max() <= 1e-10, np.abs(total - lens).max()
    h.close()

"""Surface records on the GPU (acn_surface_rays / acn_surface_positions, include/actinon_hip.h) against the CPU model of
tests/surface_model.py, which test_surface_cpu.py pins to the oracle: the oracle's scene hit, its obj_color read off an
emissive copy of the scene, and the FOLLOW rule restated with the reference's expression order.  Everything is compared bit
for bit; what the model cannot decide (two branch shares within 1e-9 of each other, a texture coordinate within 1e-9 of a
cell boundary) is left out, and the tests bound how much that may be."""
import os
import subprocess
import sys

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
import surface_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["hanging_lamp", "paraffin_lamp", "ruby_heart", "pyramid"]
TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def load(name):
    if name in S.SMALL:
        return S.build(name)[1]
    return A.Flat.load(os.path.join(ROOT, "tests", "golden", "scenes", name + ".npz"), image_width=64, image_height=48)


def assert_first_hit(got, model, rays):
    """slots 0, 4 - 8 and the kind bits equal the model's, the position is p + d * a, hops 0, weight 1, slot 15 zero"""
    hit = model[:, 0] < np.inf
    for k in (0, 4, 5, 6, 7, 8, 12):
        bad = np.flatnonzero(got[:, k] != model[:, k])
        assert len(bad) == 0, (k, bad[:5], got[bad[:5], k], model[bad[:5], k])
    assert np.array_equal(got[hit, 1:4], rays[hit, :3] + rays[hit, 3:] * got[hit, :1])
    assert (got[~hit, 1:7] == 0).all() and (got[~hit, 9:13] == 0).all()
    assert (got[:, 13] == 0).all() and (got[:, 14] == 1).all() and (got[:, 15] == 0).all()


@pytest.mark.parametrize("name", list(S.SMALL) + FIXTURES)
def test_first_hit_is_the_oracles(oracle, name):
    flat = load(name)
    pos = S.positions(flat)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    s = h.surface_positions(pos)
    h.close()
    model, _ = M.first_hit(oracle, flat, rays)
    assert_first_hit(s.raw, model, rays)
    assert s.hit.sum() >= 0.3 * len(pos)


def assert_albedo(oracle, flat, pos, got, min_enter):
    """the device's colour is, bit for bit, the colour of the texture (or the node) that the oracle chose; returns per row
    the node and which colour that was"""
    en = got[:, 7].astype(np.int64)
    sel = (got[:, 0] < np.inf) & (en >= 0)
    assert sel.sum() >= min_enter
    alb = M.oracle_albedo(oracle, flat, pos, en, got[:, 1:4])
    exact, which = M.exact_colour(flat, en[sel], alb[sel], TOL)
    bad = np.flatnonzero((exact != got[sel, 9:12]).any(axis=1))
    assert len(bad) == 0, (bad[:5], exact[bad[:5]], got[sel][bad[:5], 9:12])
    return en[sel], which, got[sel, 12].astype(np.int64)


def chess_nodes(flat, node_type):
    return [i for i in range(flat.n_nodes) if flat.node(i).type == node_type and flat.node(i).texture >= 0
            and flat.c.textures[flat.node(i).texture].kind == 1]      # ACN_TXM_CHESS


@pytest.mark.parametrize("name", ["textured", "wine_glass_c2", "primitives_c1"])
def test_albedo_is_the_oracles_obj_color(oracle, name):
    sc, flat = S.build(name)
    pos = S.positions(flat)
    h = A.Handle(flat)
    got = h.surface_positions(pos).raw
    h.close()
    node, which, kind = assert_albedo(oracle, flat, pos, got, 1000)
    if name != "textured":
        return
    radiance = np.array([flat.node(i).radiance for i in range(flat.n_nodes)])
    (plane,) = chess_nodes(flat, A.abi.ACN_PLANE)
    balls = chess_nodes(flat, A.abi.ACN_SPHERE)
    (ball,) = [b for b in balls if radiance[b] == 0]
    (light,) = [b for b in balls if radiance[b] > 0]
    for nd in (plane, ball):
        assert (which[node == nd] == 1).sum() >= 100 and (which[node == nd] == 2).sum() >= 100, nd
    assert (node == light).sum() == 0          # the scene's camera does not see the light: a second camera that does
    lp = np.array(flat.node(light).pos[:])
    cp = np.array(flat.params.camera_position[:])
    sc.set(camera_view_direction=lp - cp, camera_focal_length=6.0, image_width=64, image_height=48)
    cam = sc.flatten()
    pos = S.positions(cam)
    h = A.Handle(cam)
    got = h.surface_positions(pos).raw
    h.close()
    node, which, kind = assert_albedo(oracle, cam, pos, got, 200)
    on = node == light
    assert (which[on] == 1).sum() >= 50 and (which[on] == 2).sum() >= 50
    assert (kind[on] & (M.LIGHT_ROOT | M.EMITTER) == (M.LIGHT_ROOT | M.EMITTER)).all()
    assert (kind[~on] & M.LIGHT_ROOT == 0).all()


@pytest.mark.parametrize("name", ["wine_glass_c2", "textured"])
def test_positions_are_their_camera_rays(name):
    """surface_positions( pos ) == surface_rays( camera_rays( pos ) ) bit for bit: host buffers, and the device entry points
    on a torch stream of the caller's, into a NaN-filled buffer whose row behind n stays as it was"""
    import torch
    sc, flat = S.build(name)
    pos = S.positions(flat)
    n = len(pos)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    for follow in (False, True):
        by_pos = h.surface_positions(pos, follow=follow).raw
        by_ray = h.surface_rays(rays, follow=follow).raw
        assert np.array_equal(by_pos, by_ray), follow
        assert not np.isnan(by_pos).any()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_pos = torch.from_numpy(pos).to("cuda")
            d_rays = torch.from_numpy(rays).to("cuda")
            d_a = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
            d_b = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
            assert d_a.data_ptr() % 128 == 0 and d_b.data_ptr() % 128 == 0
            h.surface_positions_dev(d_pos.data_ptr(), n, d_a.data_ptr(), follow=follow, stream=s.cuda_stream)
            h.surface_rays_dev(d_rays.data_ptr(), n, d_b.data_ptr(), follow=follow, stream=s.cuda_stream)
        s.synchronize()
        a, b = d_a.cpu().numpy(), d_b.cpu().numpy()
        assert np.array_equal(a[:n], by_pos) and np.array_equal(b[:n], by_pos), follow
        assert np.isnan(a[n]).all() and np.isnan(b[n]).all()
    h.close()


def test_rays_that_start_inside_matter(oracle):
    """the inside cameras of test_gpu_rays.FOREIGN (inside the wine, the stone, the chess ball) at 32x20, focal length 1"""
    from test_gpu_rays import FOREIGN
    for name in ("wine_glass_c2", "diamond_c4", "textured"):
        sc, flat = S.build(name)
        p, tgt, top, focal, w, hh = FOREIGN[name][2]
        sc.set(camera_position=p, camera_view_direction=np.subtract(tgt, p), camera_top_direction=top, camera_focal_length=1.0,
               image_width=32, image_height=20)
        cam = sc.flatten()
        pos = S.positions(cam)
        h = A.Handle(cam)
        rays = h.camera_rays(pos)
        got = h.surface_rays(rays).raw
        h.close()
        model, edge = M.first_hit(oracle, cam, rays)
        assert_first_hit(got, model, rays)
        en, ex = got[:, 7].astype(np.int64), got[:, 8].astype(np.int64)
        assert (ex >= 0).sum() >= 100, name
        if name == "wine_glass_c2":
            assert ((ex >= 0) & (en >= 0)).sum() >= 100      # wine to glass
        if (en >= 0).any():
            assert_albedo(oracle, cam, pos, got, 1)
        only_exit = (got[:, 0] < np.inf) & (en < 0)
        assert (only_exit & edge).sum() <= 0.001 * len(pos)
        use = only_exit & ~edge
        assert np.array_equal(got[use, 9:12], model[use, 9:12]), name


@pytest.mark.parametrize("name", ["wine_glass_c2", "diamond_c4", "paraffin_lamp", "pyramid", "textured"])
def test_follow_is_the_models_chain(oracle, name):
    flat = load(name)
    pos = S.positions(flat)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    got = h.surface_positions(pos, follow=True).raw
    first = h.surface_positions(pos).raw
    h.close()
    model, tie = M.follow(oracle, flat, rays)
    assert tie.mean() <= 0.005, tie.mean()
    use = ~tie
    bad = np.flatnonzero(use & (got != model).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], model[bad[:5]])
    hops = got[use, 13]
    kind = got[use, 12].astype(np.int64)
    assert (hops > 0).mean() >= 0.05, (hops > 0).mean()
    assert ((got[use, 0] == np.inf) & (hops > 0)).sum() >= 1
    if name == "wine_glass_c2":
        assert ((kind & M.CUT) != 0).sum() >= 1
    same = got[:, 13] == 0
    assert np.array_equal(got[same], first[same])


def test_records_do_not_depend_on_wave_neighbours():
    sc, flat = S.build("wine_glass_c2")
    h = A.Handle(flat)
    rays = h.camera_rays(S.positions(flat))
    perm = np.random.default_rng(17).permutation(len(rays))
    for follow in (False, True):
        plain = h.surface_rays(rays, follow=follow).raw
        back = np.empty_like(plain)
        back[perm] = h.surface_rays(rays[perm], follow=follow).raw
        assert np.array_equal(back, plain), follow
        k = 1000                                       # a short call: a partly filled last wave
        assert np.array_equal(h.surface_rays(rays[:k + 37], follow=follow).raw, plain[:k + 37])
    h.close()


def test_contract_of_a_surface_call():
    import ctypes as C
    import torch
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)[::7]
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    n = len(rays)
    stream = torch.cuda.current_stream().cuda_stream
    assert h.surface_rays(np.zeros((0, 6))).raw.shape == (0, 16)
    assert h.surface_positions(np.zeros((0, 2)), follow=True).raw.shape == (0, 16)
    sentinel = torch.full((n, 16), 7.25, dtype=torch.float64, device="cuda")
    h.surface_rays_dev(0, 0, sentinel.data_ptr(), stream=stream)
    h.surface_positions_dev(0, 0, sentinel.data_ptr(), stream=stream)
    d_bad = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    for i, j, v in ((37, 3, np.nan), (5, 0, np.inf), (12, None, 0.0)):
        bad = rays.copy()
        if j is None:
            bad[i, 3:] = 0.0
        else:
            bad[i, j] = v
        bad[n - 1, 4] = np.nan                           # a second refused ray: the first one is named
        for follow in (False, True):
            with pytest.raises(A.AcnError) as e:
                h.surface_rays(bad, follow=follow)
            assert e.value.status == A.abi.ACN_ERR_ARG and f"ray {i}:" in str(e.value), str(e.value)
            d_bad.copy_(torch.from_numpy(bad))
            with pytest.raises(A.AcnError) as e:
                h.surface_rays_dev(d_bad.data_ptr(), n, sentinel.data_ptr(), follow=follow, stream=stream)
            assert e.value.status == A.abi.ACN_ERR_ARG and f"ray {i}:" in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert (sentinel == 7.25).all()
    out = np.full((n, 16), 7.25)
    o = A.abi.RenderOpts()
    o.struct_size = C.sizeof(A.abi.RenderOpts)
    for fn, src in ((A.hip.acn_surface_rays, rays), (A.hip.acn_surface_positions, pos)):
        assert fn(h.h, src.ctypes.data, n, 7, out.ctypes.data, C.byref(o)) == A.abi.ACN_ERR_ARG
        assert b"mode" in A.hip.acn_last_error()
        o.shard_mode, o.shard_rank, o.shard_world = A.abi.ACN_SHARD_SAMPLES, 0, 2
        assert fn(h.h, src.ctypes.data, n, 0, out.ctypes.data, C.byref(o)) == A.abi.ACN_ERR_ARG
        o.shard_mode, o.shard_rank, o.shard_world = A.abi.ACN_SHARD_NONE, 0, 0
    d_rays = torch.from_numpy(rays).to("cuda")
    o.stream = stream
    assert A.hip.acn_surface_rays_dev(h.h, d_rays.data_ptr(), n, 7, sentinel.data_ptr(), C.byref(o)) == A.abi.ACN_ERR_ARG
    o.shard_world = 2
    assert A.hip.acn_surface_rays_dev(h.h, d_rays.data_ptr(), n, 1, sentinel.data_ptr(), C.byref(o)) == A.abi.ACN_ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.25).all() and (sentinel == 7.25).all()
    # directions of any length are scaled by 1 / sqrt( x*x + y*y + z*z ) (v3d_s_of_length)
    long = rays.copy()
    long[:, 3:] *= 2.5
    x, y, z = long[:, 3], long[:, 4], long[:, 5]
    unit = long.copy()
    unit[:, 3:] = long[:, 3:] * (1 / np.sqrt(x * x + y * y + z * z))[:, None]
    assert np.array_equal(h.surface_rays(long, follow=True).raw, h.surface_rays(unit, follow=True).raw)
    h.close()


def test_a_surface_call_leaves_the_renderer_alone():
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    h = A.Handle(flat)
    before = h.render_positions(pos, linear=True)
    st0 = h.last_stages()
    rays = h.camera_rays(pos)
    for follow in (False, True):
        h.surface_positions(pos, follow=follow)
        h.surface_rays(rays, follow=follow)
    after = h.render_positions(pos, linear=True)
    st1 = h.last_stages()
    h.close()
    assert np.array_equal(before, after)
    assert st1["retries"] == 0 and st1["workspace_allocs"] == st0["workspace_allocs"], (st0, st1)


def test_pick_and_the_aov_tool(oracle, tmp_path, monkeypatch):
    sc, flat = S.build("textured")
    pos = S.positions(flat)
    h = A.Handle(flat)
    rays = h.camera_rays(pos)
    model, _ = M.first_hit(oracle, flat, rays)
    hit = model[:, 0] < np.inf
    assert hit.any() and (~hit).any()
    i, j = np.flatnonzero(hit)[len(np.flatnonzero(hit)) // 2], np.flatnonzero(~hit)[0]
    assert h.pick(pos[j, 0], pos[j, 1]) is None
    got = h.pick(pos[i, 0], pos[i, 1])
    node = int(model[i, 7]) if model[i, 7] >= 0 else int(model[i, 8])
    assert got["node"] == node and got["type"] == A.abi.NODE_TYPES[flat.node(node).type]
    assert got["distance"] == model[i, 0] and np.array_equal(got["position"], model[i, 1:4])
    h.close()

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_aovs as T
    from render_panorama import load_scene
    script = os.path.join(ROOT, "tests", "scripts", "csg.acn")
    for follow in (False, True):
        out = tmp_path / ("follow" if follow else "first")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_aovs.py"), script, str(out)] + (["--follow"] if follow else []),
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(out)) == ["albedo.pnm", "depth.pfm", "normal.pnm", "object_id.pgm", "surface.npy"]
        monkeypatch.chdir(tmp_path)
        f = load_scene(script)
        w, hh = int(f.params.image_width), int(f.params.image_height)
        hd = A.Handle(f)
        s = hd.surface_positions(A.main_pass_positions(w, hh), follow=follow)
        hd.close()
        assert s.hit.any()
        assert np.array_equal(np.load(out / "surface.npy"), s.raw)
        depth, normal, albedo, ids = T.aov_images(s, w, hh)
        assert np.array_equal(T.read_pfm(out / "depth.pfm"), depth)
        assert np.array_equal(T.read_pnm(out / "normal.pnm"), normal)
        assert np.array_equal(T.read_pnm(out / "albedo.pnm"), albedo)
        assert np.array_equal(T.read_pnm(out / "object_id.pgm"), ids) and ids.max() > 0

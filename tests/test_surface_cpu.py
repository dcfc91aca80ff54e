"""Surface records without a GPU: the refusals that need no device, the CPU model of tests/surface_model.py against the oracle
(so that test_gpu_surface.py compares the device with something the oracle vouches for), the image writers of
tools/render_aovs.py, and the Surface views."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import scenes_util as S
import surface_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TOL = 1e-9


@pytest.mark.parametrize("fn", ["acn_surface_rays", "acn_surface_rays_dev", "acn_surface_positions", "acn_surface_positions_dev"])
def test_null_handle_is_refused(fn):
    buf = np.zeros((4, 16))
    o = A.abi.RenderOpts()
    o.struct_size = C.sizeof(A.abi.RenderOpts)
    for opts in (None, C.byref(o)):
        st = getattr(A.hip, fn)(None, buf.ctypes.data, 2, A.abi.ACN_SURF_FIRST_HIT, buf.ctypes.data, opts)
        assert st == A.abi.ACN_ERR_ARG
        assert b"null" in A.hip.acn_last_error()
    assert (buf == 0).all()


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    for name in ("STRIDE", "FIRST_HIT", "FOLLOW", "EMITTER", "DIFFUSE", "CHROMATIC", "FRESNEL", "TRANSPARENT", "LIGHT_ROOT", "CUT"):
        line = [ln for ln in text.splitlines() if ln.startswith(f"#define ACN_SURF_{name} ")]
        assert len(line) == 1, name
        assert int(line[0].split()[2].rstrip("u")) == getattr(A.abi, "ACN_SURF_" + name), name
    assert (M.EMITTER, M.DIFFUSE, M.CHROMATIC, M.FRESNEL, M.TRANSPARENT, M.LIGHT_ROOT, M.CUT, M.STRIDE) == (
        A.abi.ACN_SURF_EMITTER, A.abi.ACN_SURF_DIFFUSE, A.abi.ACN_SURF_CHROMATIC, A.abi.ACN_SURF_FRESNEL,
        A.abi.ACN_SURF_TRANSPARENT, A.abi.ACN_SURF_LIGHT_ROOT, A.abi.ACN_SURF_CUT, A.abi.ACN_SURF_STRIDE)


@pytest.mark.parametrize("name", ["wine_glass_c2", "diamond_c4", "textured", "primitives_path"])
def test_model_hit_is_the_oracles_scene_hit(oracle, name):
    """two batch calls, matter winning only if strictly nearer == the scalar scene_s_trans_hit of the oracle"""
    sc, flat = S.build(name)
    rays = M.camera_rays(flat.params, S.positions(flat))
    a, nor, ex, en, light = M.scene_hit(oracle, flat, rays)
    hits = 0
    for i in range(0, len(rays), max(1, len(rays) // 400)):
        a1, n1, ex1, en1 = oracle.trans_hit(flat, rays[i, :3], rays[i, 3:])
        if a1 < np.inf:
            hits += 1
            assert a1 == a[i] and ex1 == ex[i] and en1 == en[i] and np.array_equal(n1, nor[i]), i
        else:
            assert np.isinf(a[i]) and ex[i] == -1 and en[i] == -1, i
    assert hits >= 100
    rec, _ = M.first_hit(oracle, flat, rays)
    hit = rec[:, 0] < np.inf
    assert np.array_equal(rec[hit, 1:4], rays[hit, :3] + rays[hit, 3:] * rec[hit, :1])
    assert (rec[~hit, 1:13] == np.array([0] * 6 + [-1, -1] + [0] * 4)).all() and (rec[:, 14] == 1).all()


@pytest.mark.parametrize("name", ["textured", "wine_glass_c2"])
def test_model_albedo_is_the_oracles_obj_color(oracle, name):
    """numpy obj_color against the oracle's, read off an emissive copy of the scene (surface_model.oracle_albedo)"""
    sc, flat = S.build(name)
    pos = S.positions(flat)
    rays = M.camera_rays(flat.params, pos)
    rec, edge = M.first_hit(oracle, flat, rays)
    en = rec[:, 7].astype(np.int64)
    sel = (rec[:, 0] < np.inf) & (en >= 0)
    assert sel.sum() >= 1000
    alb = M.oracle_albedo(oracle, flat, pos, en, rec[:, 1:4])
    use = sel & ~edge
    assert (sel & edge).sum() <= 0.001 * sel.sum()
    assert np.abs(alb[use] - rec[use, 9:12]).max() <= TOL
    exact, which = M.exact_colour(flat, en[use], alb[use])
    assert np.array_equal(exact, rec[use, 9:12])
    if name == "textured":
        _, mwhich, _ = M.obj_color_model(flat, en[use], rec[use, 1:4])
        assert np.array_equal(which, mwhich)
        chess = [i for i in range(flat.n_nodes) if flat.node(i).texture >= 0 and flat.c.textures[flat.node(i).texture].kind == 1]
        both = [i for i in chess if {1, 2} <= set(which[en[use] == i])]
        assert len(both) >= 2, (chess, both)      # the chess plane and the chess ball show both colours


def test_model_follow_reaches_through_glass(oracle):
    """the chain of the model on the headline scene: rays that cross the glass end on a diffuse surface behind it"""
    sc, flat = S.build("wine_glass_c2")
    rays = M.camera_rays(flat.params, S.positions(flat))
    first, _ = M.first_hit(oracle, flat, rays)
    rec, tie = M.follow(oracle, flat, rays)
    hops = rec[:, 13]
    assert tie.mean() <= 0.005
    assert (hops > 0).mean() >= 0.05 and hops.max() <= flat.params.trace_depth - 1
    same = hops == 0
    assert np.array_equal(rec[same], first[same])
    kind = rec[:, 12].astype(np.int64)
    ends = (rec[:, 0] < np.inf) & ~tie
    stop = (kind & (M.EMITTER | M.DIFFUSE | M.CUT)) != 0
    glass = ends & (hops > 0)
    assert (stop[glass]).mean() > 0.9
    assert ((kind & M.CUT) != 0).sum() >= 1 and (hops[(kind & M.CUT) != 0] == flat.params.trace_depth - 1).all()
    assert ((rec[:, 0] == np.inf) & (hops > 0)).sum() >= 1
    assert (rec[:, 14] <= 1).all() and (rec[hops > 0, 14] < 1).all() and (rec[:, 14] > 0).all()


def test_image_writers_round_trip(tmp_path):
    import render_aovs as T
    rng = np.random.default_rng(3)
    depth = rng.uniform(0.1, 30, (5, 7)).astype(np.float32)
    depth[1, 2] = np.inf
    T.write_pfm(tmp_path / "d.pfm", depth)
    assert np.array_equal(T.read_pfm(tmp_path / "d.pfm"), depth)
    assert (tmp_path / "d.pfm").read_bytes().startswith(b"Pf\n7 5\n-1.0\n")
    col = rng.uniform(0, 1, (5, 7, 3)).astype(np.float32)
    T.write_pfm(tmp_path / "c.pfm", col)
    assert np.array_equal(T.read_pfm(tmp_path / "c.pfm"), col)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    T.write_pnm(tmp_path / "c.pnm", rgb)
    assert np.array_equal(T.read_pnm(tmp_path / "c.pnm"), rgb)
    ids = rng.integers(0, 65536, (5, 7)).astype(np.uint16)
    ids[0, 0], ids[0, 1] = 0, 65535
    T.write_pgm16(tmp_path / "i.pgm", ids)
    assert np.array_equal(T.read_pnm(tmp_path / "i.pgm"), ids)
    assert (tmp_path / "i.pgm").read_bytes()[:len(b"P5\n7 5\n65535\n")] == b"P5\n7 5\n65535\n"
    with pytest.raises(ValueError):
        T.write_pgm16(tmp_path / "x.pgm", np.array([[70000]]))
    with pytest.raises(ValueError):
        T.write_pnm(tmp_path / "x.pnm", col)


def test_aov_images_of_hand_made_records(tmp_path):
    import render_aovs as T
    raw = M.blank(6)
    raw[1] = [2.5, 1, 2, 3, 0, 0, -1, 4, -1, 0.25, 0.5, 1.0, 2, 0, 1, 0]
    raw[4] = [7.0, 0, 0, 1, 1, 0, 0, -1, 9, 0.0, 1.0, 0.5, 24, 3, 0.4, 0]
    s = A.Surface(raw)
    T.write_aovs(str(tmp_path), s, 3, 2)
    depth = T.read_pfm(tmp_path / "depth.pfm")
    assert depth.shape == (2, 3) and depth[0, 1] == 2.5 and depth[1, 1] == 7.0 and np.isinf(depth[0, 0])
    ids = T.read_pnm(tmp_path / "object_id.pgm")
    assert ids.tolist() == [[0, 5, 0], [0, 10, 0]]
    nrm = T.read_pnm(tmp_path / "normal.pnm")
    assert nrm[0, 1].tolist() == [128, 128, 255] and nrm[1, 1].tolist() == [0, 128, 128] and nrm[0, 0].tolist() == [0, 0, 0]
    alb = T.read_pnm(tmp_path / "albedo.pnm")
    assert alb[0, 1].tolist() == [64, 128, 255] and alb[1, 1].tolist() == [0, 255, 128]
    assert np.array_equal(np.load(tmp_path / "surface.npy"), raw)


def test_surface_views():
    raw = M.blank(3)
    raw[1] = [2.5, 1, 2, 3, 0, 0.6, -0.8, 4, -1, 0.25, 0.5, 1.0, 2, 0, 1, 0]
    raw[2] = [7.0, 0, 0, 1, 1, 0, 0, -1, 9, 0.0, 1.0, 0.5, 24 + 64, 3, 0.4, 0]
    s = A.Surface(raw)
    assert len(s) == 3 and s.raw is raw
    assert s.hit.tolist() == [False, True, True] and s.hit.dtype == bool
    assert s.distance.tolist() == [np.inf, 2.5, 7.0]
    assert s.position[1].tolist() == [1, 2, 3]
    assert s.exit_normal[1].tolist() == [0, 0.6, -0.8] and s.normal[1].tolist() == [0, -0.6, 0.8]
    assert s.enter.tolist() == [-1, 4, -1] and s.exit.tolist() == [-1, -1, 9] and s.enter.dtype == np.int64 and s.exit.dtype == np.int64
    assert s.albedo[2].tolist() == [0.0, 1.0, 0.5]
    assert s.kind.tolist() == [0, 2, 88] and s.kind[2] & A.abi.ACN_SURF_CUT
    assert s.hops.tolist() == [0, 0, 3] and s.weight.tolist() == [1.0, 1.0, 0.4]
    with pytest.raises(ValueError):
        A.Surface(np.zeros((3, 5)))

"""acn_shadow_records* and acn_shadow_limit_history* on the GPU (include/actinon_hip.h).

Records: all sixteen doubles, bit for bit, against the oracle's tap (tests/shadow_model.py; test_shadow_cpu.py checks the tap by two
one-ray queries) on eight handles -- the five small configurations, one scene with three lights, so that the stream offset i * S
counts, and two handles whose nodes are staged in LDS -- at about 600 positions each: a stride over the raster plus a dense window over a cast shadow, chosen on the CPU with the oracle
alone, so that penumbra and umbra are both there; the counts are asserted.  NONE records, independence of how records are packed
into wavefronts for every S, both node arrangements, every refusal, the handle left as found.  The guard: against the numpy model,
bit for bit, on the hand-made arrays and on a real pair of frames."""
import ctypes as C
import math

import numpy as np
import pytest

import actinon_amd as A
import lens_layers_model as Y
import motion_model as MM
import ray_sets as R
import scenes_util as S
import shadow_model as SM
import surface_model as M
from actinon_amd import abi
from actinon_amd._lib import hip, host
from actinon_amd.motion import rigid_copy
from query_checks import upload

pytestmark = pytest.mark.gpu
SCENES = ["primitives_c1", "textured", "wine_glass_c2", "diamond_c4", "many_spheres_c3", "three_lights", "textured_lds", "small_scene"]
ALL_S = [1, 2, 4, 8, 16, 32, 64]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


def assert_same_bits(got, want):
    bad = Y.same_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def build_three_lights():
    """build_textured's objects and two more sphere lights: three elements in the light root"""
    sc = S.build_textured()
    for radius, radiance, at in ((0.4, 18.0, (3.0, -2.0, 4.0)), (0.8, 12.0, (0.5, 4.0, 6.0))):
        light = host.acn_obj_sphere_s_create(radius)
        host.acn_obj_set_radiance(light, radiance)
        host.acn_obj_move(light, A.v3(*at))
        sc.push(light)
        host.acn_obj_discard(light)
    return sc, sc.flatten()


def build(name):
    """small_scene: a dozen nodes with a generic compound at the matter root, which the upload stages in LDS (ray_sets.walk_small_scene);
    textured_lds: `textured`, uploaded with its nodes forced into LDS"""
    if name == "three_lights":
        return build_three_lights()
    if name == "small_scene":
        return R.walk_small_scene()
    return S.build("textured" if name == "textured_lds" else name)


def choose_positions(orc, flat, n_stride=400, n_edge=150, n_dark=50):
    """About 600 sample positions: a stride over a grid of the whole raster, and the grid points of a cast shadow -- where the ray
    from the first hit to the centre of a light is occluded -- with the points along its edge.  The oracle alone decides."""
    W, H = int(flat.params.image_width), int(flat.params.image_height)
    g = max(0.25, math.sqrt(W * H / 24000.0))
    xs, ys = np.arange(g / 2, W, g), np.arange(g / 2, H, g)
    grid = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    rays = M.camera_rays(flat.params, grid)
    surf, _ = M.first_hit(orc, flat, rays)
    ok = SM.sampled(surf) & ((surf[:, 12].astype(np.int64) & M.DIFFUSE) != 0)
    lights = flat.node(flat.c.light_root)
    occ = np.zeros(len(grid), bool)
    for k in range(lights.child1):
        centre = np.array(flat.node(flat.c.elems[lights.child0 + k]).pos[:])
        d = centre[None, :] - surf[:, 1:4]
        dist = np.sqrt((d * d).sum(1))
        d = d / np.where(dist > 0, dist, 1.0)[:, None]
        facing = ok & (M.dot(d, -surf[:, 4:7]) > 0)
        idx = np.flatnonzero(facing)
        q = np.concatenate([surf[idx, 1:4], d[idx]], axis=1)
        occ[idx] |= orc.query_rays(flat, "occluded", flat.c.matter_root, q, limits=dist[idx])[:, 5] != 0
    o2, k2 = occ.reshape(len(ys), len(xs)), ok.reshape(len(ys), len(xs))
    edge = np.zeros_like(o2)
    for ax, sh in ((0, 1), (0, -1), (1, 1), (1, -1)):
        edge |= k2 & np.roll(k2, sh, axis=ax) & (o2 != np.roll(o2, sh, axis=ax))
    edge = edge.reshape(-1)
    dark = occ & ~edge
    pick = lambda idx, n: idx[::max(1, len(idx) // n)][:n] if len(idx) else idx
    chosen = np.unique(np.concatenate([pick(np.arange(len(grid)), n_stride), pick(np.flatnonzero(edge), n_edge), pick(np.flatnonzero(dark), n_dark)]))
    return np.ascontiguousarray(grid[chosen])


_DATA = {}


def scene_data(name, orc):
    """one handle per scene, its positions, the device's rays and first-hit records, and the tap's records at S = 8: made once"""
    if name not in _DATA:
        sc, flat = build(name)
        h = upload(flat, ACN_LDS_MAX=40960) if name == "textured_lds" else A.Handle(flat)
        pos = choose_positions(orc, flat)
        rays = h.camera_rays(pos)
        surf = h.surface_positions(pos).raw
        _DATA[name] = dict(sc=sc, flat=flat, h=h, pos=pos, rays=rays, surf=surf, lds=h.stage_info()["lds_nodes"], want={})
    return _DATA[name]


def tap_records(d, orc, samples):
    if samples not in d["want"]:
        d["want"][samples] = SM.records_from_tap(orc, d["flat"], d["rays"], d["surf"], samples)
    return d["want"][samples]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for d in _DATA.values():
        d["h"].close()
    _DATA.clear()


def records_dev(h, surf, samples, stream=None):
    """the _dev form on torch buffers with a NaN record behind the output -> the records read back"""
    import torch
    n = len(surf)
    d_in = torch.from_numpy(np.ascontiguousarray(surf)).to("cuda")
    d_out = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.shadow_records_dev(d_in.data_ptr(), n, d_out.data_ptr(), samples=samples, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[-1]).all()
    assert np.array_equal(d_in.cpu().numpy(), surf)
    return out[:-1]


# ---- 1, 4: the records against the tap ----
@pytest.mark.parametrize("name,samples", [(n, 8) for n in SCENES] + [("primitives_c1", 1), ("textured", 64), ("three_lights", 64)])
def test_records_are_the_taps_bit_for_bit(oracle, name, samples):
    d = scene_data(name, oracle)
    surf = d["surf"]
    assert 500 <= len(surf) <= 700
    got = d["h"].shadow_records(surf, samples)
    want, compared = tap_records(d, oracle, samples)
    hits = surf[:, 0] < np.inf
    on = SM.sampled(surf)
    assert np.array_equal(got[:, 0], on.astype(np.float64))
    assert (got[on, 1] == samples).all() and (got[on, 2] == d["flat"].node(d["flat"].c.light_root).child1).all()
    bad = np.flatnonzero(compared & ~(got == want).all(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    asked, clear = got[:, 3], got[:, 4]
    partial, dark = int(((clear > 0) & (clear < asked)).sum()), int(((clear == 0) & (asked > 0)).sum())
    print(f"{name} S={samples}: {int(compared.sum())} of {int(hits.sum())} hit records compared ({compared.sum() / hits.sum():.3f}); "
          f"{partial} partly lit, {dark} dark; nodes in LDS: {d['lds']}")
    assert compared.sum() >= 0.9 * hits.sum()
    if samples == 8:
        assert partial >= 32 and dark >= 8
    assert_same_bits(records_dev(d["h"], surf, samples), got)                 # the _dev form


def test_both_node_arrangements_were_compared(oracle):
    staged = {name: scene_data(name, oracle)["lds"] for name in SCENES}
    assert staged["textured_lds"] and staged["small_scene"] and not staged["textured"] and not staged["wine_glass_c2"], staged
    assert scene_data("three_lights", oracle)["flat"].node(scene_data("three_lights", oracle)["flat"].c.light_root).child1 == 3


# ---- 2: NONE ----
def test_none_records_are_sixteen_zeros(oracle):
    d = scene_data("textured", oracle)
    surf, h = d["surf"], d["h"]
    sky = ~(surf[:, 0] < np.inf)
    assert sky.sum() >= 10
    got = h.shadow_records(surf, 8)
    assert (got[sky] == 0).all() and (got[~sky, 0] == 1).all()
    # hand-made: a hit with [ 0 ] = inf, a hit with the EMITTER bit, a NaN distance
    k = np.flatnonzero(~sky)[:64]
    hand = np.repeat(surf[k], 4, axis=0)
    hand[1::4, 0] = np.inf
    hand[2::4, 12] = hand[2::4, 12] + abi.ACN_SURF_EMITTER
    hand[3::4, 0] = np.nan
    out = h.shadow_records(hand, 8)
    assert np.array_equal(out[0::4], got[k])
    assert (out[1::4] == 0).all() and (out[2::4] == 0).all() and (out[3::4] == 0).all()
    # a camera aimed at the light: the records carry the EMITTER bit
    flat = d["flat"]
    light = flat.node(flat.c.elems[flat.node(flat.c.light_root).child0])
    hd = A.Handle(flat)
    try:
        cam = np.array(hd.params.camera_position[:])
        hd.set_params(camera_view_direction=tuple(np.array(light.pos[:]) - cam))
        W, H = hd.params.image_width, hd.params.image_height
        pos = np.array([[W / 2 + dx, H / 2 + dy] for dx in (-1.5, -0.5, 0.5, 1.5) for dy in (-1.5, -0.5, 0.5, 1.5)])
        at_light = hd.surface_positions(pos).raw
        assert (at_light[:, 0] < np.inf).all() and ((at_light[:, 12].astype(np.int64) & abi.ACN_SURF_EMITTER) != 0).all()
        assert (hd.shadow_records(at_light, 8) == 0).all()
    finally:
        hd.close()


# ---- 3: independence of packing ----
@pytest.mark.parametrize("samples", ALL_S)
def test_a_record_does_not_depend_on_its_wavefront(oracle, samples):
    d = scene_data("wine_glass_c2", oracle)
    surf, h = d["surf"], d["h"]
    rng = np.random.default_rng(11)
    hit = np.flatnonzero(surf[:, 0] < np.inf)
    recs = surf[rng.choice(hit, 1000)].copy()
    none_at = np.unique(np.concatenate([rng.integers(0, 1000, 120), [0, 5, 6, 7, 63, 64, 65, 999]]))
    recs[none_at] = M.blank(len(none_at))
    full = h.shadow_records(recs, samples)
    assert (full[none_at] == 0).all() and (np.delete(full, none_at, axis=0)[:, 0] == 1).all()
    assert ((full[:, 3] > 0) & (full[:, 4] == 0)).sum() >= 10 and ((full[:, 3] > 0) & (full[:, 4] == full[:, 3])).sum() >= 10
    assert samples == 1 or ((full[:, 4] > 0) & (full[:, 4] < full[:, 3])).sum() >= 10
    assert np.array_equal(h.shadow_records(recs[::-1], samples), full[::-1])
    for k in (1, 63, 64 // samples + 1, 257):
        assert np.array_equal(h.shadow_records(recs[:k], samples), full[:k]), k
    if samples in (1, 16):
        assert np.array_equal(records_dev(h, recs, samples), full)


def test_the_default_is_sixteen_samples(oracle):
    d = scene_data("textured", oracle)
    surf, h = d["surf"][:100], d["h"]
    out = np.full((100, 16), np.nan)
    o = h._plain_opts(False, None)
    for prm in (None, C.byref(A.Handle.shadow_params(None))):
        assert hip.acn_shadow_records(h.h, surf.ctypes.data, 100, prm, out.ctypes.data, C.byref(o)) == abi.ACN_OK
        assert np.array_equal(out, h.shadow_records(surf, 16))


# ---- 5: refusals ----
def test_refusals_leave_the_output_untouched(oracle):
    import torch
    d = scene_data("textured", oracle)
    h = d["h"]
    n = 40
    surf = np.ascontiguousarray(d["surf"][:n])
    o = h._plain_opts(False, None)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_surf, d_out = torch.from_numpy(surf).to("cuda"), nan(n + 1, 16)
    h_out = np.full((n + 1, 16), np.nan)
    sp = A.Handle.shadow_params(8)
    # the guard's buffers
    stats, motion = np.tile(np.array([8.0, 1, 2, 3, 4, 5, 6, 0]), (n, 1)), np.full((n, 2), 1.5)
    cur = np.tile(SM.shadow_rec(8, [8], [0]), (n, 1))
    prev = np.tile(SM.shadow_rec(8, [8], [8]), (12, 1))
    h_stats, h_change = stats.copy(), np.full(n + 1, np.nan)
    d_stats, d_motion, d_cur, d_prev, d_change = [torch.from_numpy(a.copy()).to("cuda") for a in (stats, motion, cur, prev)] + [nan(n + 1)]
    gp = A.Handle.shadow_history_params()
    torch.cuda.synchronize()

    def refused(calls, word):
        for name, call in calls.items():
            hip.acn_render_positions(None, None, 0, None, None)              # (sets another message)
            assert call() == abi.ACN_ERR_ARG, (name, word)
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(h_out).all() and bool(torch.isnan(d_out).all()), name
            assert np.array_equal(h_stats, stats) and np.isnan(h_change).all(), name
            assert np.array_equal(d_stats.cpu().numpy(), stats) and bool(torch.isnan(d_change).all()), name

    ref = lambda x: None if x is None else C.byref(x)

    def rec(handle, opts, count=n, p=sp, ds=d_surf.data_ptr(), do=d_out.data_ptr(), hs=surf.ctypes.data, ho=h_out.ctypes.data):
        return {"host": lambda: hip.acn_shadow_records(handle, hs, count, ref(p), ho, C.byref(opts)),
                "dev": lambda: hip.acn_shadow_records_dev(handle, ds, count, ref(p), do, C.byref(opts))}

    def guard(handle, opts, count=n, w=4, hh=3, p=gp, dt=d_stats.data_ptr(), dm=d_motion.data_ptr(), dc=d_cur.data_ptr(), dp=d_prev.data_ptr(),
              dch=d_change.data_ptr(), ht=h_stats.ctypes.data, hm=motion.ctypes.data, hc=cur.ctypes.data, hp=prev.ctypes.data, hch=h_change.ctypes.data):
        return {"host": lambda: hip.acn_shadow_limit_history(handle, ht, hm, hc, hp, count, w, hh, ref(p), hch, C.byref(opts)),
                "dev": lambda: hip.acn_shadow_limit_history_dev(handle, dt, dm, dc, dp, count, w, hh, ref(p), dch, C.byref(opts))}

    only = lambda table_, *names: {k: v for k, v in table_.items() if k in names}
    world2 = h._plain_opts(False, None)
    world2.shard_world = 2
    # acn_shadow_records*
    refused(rec(None, o), "handle")
    refused(only(rec(h.h, o, hs=None), "host"), "surface")
    refused(only(rec(h.h, o, ho=None), "host"), "out")
    refused(only(rec(h.h, o, ds=None), "dev"), "surface")
    refused(only(rec(h.h, o, do=None), "dev"), "out")
    refused(rec(h.h, o, count=(1 << 31) + 1), "2^31")
    for kw, ptr in (("ds", d_surf.data_ptr() + 8), ("do", d_out.data_ptr() + 8)):
        refused(only(rec(h.h, o, **{kw: ptr}), "dev"), "align")
    refused(only(rec(h.h, o, ho=h_out.ctypes.data + 8), "host"), "align")
    for field, value, word in (("struct_size", 3, "struct_size"), ("flags", 1, "flags"), ("samples", 3, "samples"), ("samples", 65, "samples"),
                               ("samples", 128, "samples"), ("samples", 48, "samples")):
        bad = A.Handle.shadow_params(8)
        setattr(bad, field, value)
        refused(rec(h.h, o, p=bad), word)
    refused(rec(h.h, world2), "sharded")
    # acn_shadow_limit_history*
    refused(guard(None, o), "handle")
    for kw, word in (("ht", "stats"), ("hm", "motion"), ("hc", "cur_shadow"), ("hp", "prev_shadow")):
        refused(only(guard(h.h, o, **{kw: None}), "host"), word)
    for kw, word in (("dt", "stats"), ("dm", "motion"), ("dc", "cur_shadow"), ("dp", "prev_shadow")):
        refused(only(guard(h.h, o, **{kw: None}), "dev"), word)
    refused(guard(h.h, o, count=(1 << 31) + 1), "2^31")
    refused(guard(h.h, o, w=0), "raster")
    refused(guard(h.h, o, hh=0), "raster")
    refused(guard(h.h, o, w=1 << 31, hh=2), "2^31")
    for kw, buf in (("dt", d_stats), ("dc", d_cur), ("dp", d_prev)):
        refused(only(guard(h.h, o, **{kw: buf.data_ptr() + 8}), "dev"), "align")
    refused(only(guard(h.h, o, dm=d_motion.data_ptr() + 4), "dev"), "motion")
    refused(only(guard(h.h, o, dch=d_change.data_ptr() + 4), "dev"), "out_change")
    for field, value, word in (("struct_size", 3, "struct_size"), ("flags", 2, "flags"), ("tolerance", -1.0, "tolerance"), ("tolerance", float("inf"), "tolerance"),
                               ("tolerance", float("nan"), "tolerance"), ("changed_max_history", 0.5, "changed_max_history"),
                               ("changed_max_history", float("inf"), "changed_max_history"), ("changed_max_history", float("nan"), "changed_max_history")):
        bad = A.Handle.shadow_history_params()
        setattr(bad, field, value)
        refused(guard(h.h, o, p=bad), word)
    refused(guard(h.h, world2), "sharded")
    # nothing to do is ACN_OK and writes nothing, null buffers included
    for call in (lambda: hip.acn_shadow_records(h.h, None, 0, None, None, None), lambda: hip.acn_shadow_records_dev(h.h, None, 0, None, None, C.byref(o)),
                 lambda: hip.acn_shadow_limit_history(h.h, None, None, None, None, 0, 4, 3, None, None, None),
                 lambda: hip.acn_shadow_limit_history_dev(h.h, None, None, None, None, 0, 4, 3, None, None, C.byref(o))):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert np.isnan(h_out).all() and bool(torch.isnan(d_out).all()) and bool(torch.isnan(d_change).all())
    # and the handle works, with null parameters (16 samples) too
    assert hip.acn_shadow_records_dev(h.h, d_surf.data_ptr(), n, None, d_out.data_ptr(), C.byref(o)) == abi.ACN_OK
    torch.cuda.synchronize()
    back = d_out.cpu().numpy()
    assert np.array_equal(back[:n], h.shadow_records(surf, 16)) and np.isnan(back[n]).all()


# ---- 6: the handle is left as found ----
def test_a_shadow_call_leaves_the_handle_as_found(oracle):
    sc, flat = S.build("diamond_c4")
    h = A.Handle(flat)
    try:
        pos = S.positions(flat)
        assert len(pos) == 64 * 36
        h.render_positions(pos)                                               # (the handle learns its queue demand)
        before = h.render_positions(pos)
        surf = h.surface_positions(pos)
        info = h.info()
        rec = h.shadow_records(surf, 16)
        assert (rec[:, 0] == 1).sum() >= 500
        assert h.info() == info
        after = h.render_positions(pos)
        assert before.tobytes() == after.tobytes()
    finally:
        h.close()


# ---- 7: the guard against the numpy model ----
def guard_dev(h, stats, motion, cur, prev, w, hh, want_change=True, **params):
    import torch
    n = len(stats)
    up = lambda a, stride: torch.cat([torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).reshape(-1, stride),
                                      torch.full((1, stride), float("nan"), dtype=torch.float64)]).to("cuda")
    d_stats, d_motion, d_cur, d_prev = up(stats, 8), up(motion, 2), up(cur, 16), up(prev, 16)
    d_change = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h.shadow_limit_history_dev(d_stats.data_ptr(), d_motion.data_ptr(), d_cur.data_ptr(), d_prev.data_ptr(), n, w, hh,
                               d_change.data_ptr() if want_change else None, **params)
    torch.cuda.synchronize()
    out, change = d_stats.cpu().numpy(), d_change.cpu().numpy()
    assert np.isnan(out[-1]).all() and np.isnan(change[-1])
    for dbuf, a in ((d_motion, motion), (d_cur, cur), (d_prev, prev)):
        back = dbuf.cpu().numpy()
        assert_same_bits(back[:-1].reshape(np.shape(a)), a)
        assert np.isnan(back[-1]).all()
    return out[:-1], change[:-1]


@pytest.mark.parametrize("params", [dict(), dict(drop=True), dict(changed_max_history=4.0), dict(tolerance=0.2499), dict(tolerance=0.5, drop=True)])
def test_the_guard_on_the_hand_made_arrays(oracle, params):
    h = scene_data("textured", oracle)["h"]
    c = SM.hand_case()
    # 131 positions: the cases tiled over a wavefront boundary and a tail
    idx = np.arange(131) % len(c["rows"])
    stats, motion, cur = c["stats"][idx], c["motion"][idx], c["cur"][idx]
    want, want_change = SM.limit_history(stats, motion, cur, c["prev"], SM.W_HAND, SM.H_HAND, **params)
    if not params or params == dict(drop=True) or params == dict(changed_max_history=4.0):
        by_hand, by_hand_change = SM.hand_answers(drop=params.get("drop", False), cap=params.get("changed_max_history"))
        assert_same_bits(want, by_hand[idx])
        assert_same_bits(want_change, by_hand_change[idx])
    got, change = h.shadow_limit_history(stats, motion, cur, c["prev"], SM.W_HAND, SM.H_HAND, **params)
    assert_same_bits(got.raw, want)
    assert_same_bits(change, want_change)
    got, change = guard_dev(h, stats, motion, cur, c["prev"], SM.W_HAND, SM.H_HAND, **params)
    assert_same_bits(got, want)
    assert_same_bits(change, want_change)
    got, _ = guard_dev(h, stats, motion, cur, c["prev"], SM.W_HAND, SM.H_HAND, want_change=False, **params)
    assert_same_bits(got, want)


def test_the_guard_on_a_real_pair_of_frames(oracle):
    """textured at 96 x 72 with the chess ball shifted by rigid_copy: reproject_moving's history and motion, the shadow records of both
    frames at S = 16.  The floor the ball's shadow left or reached is limited, the floor far from it is not; a resting pair changes nothing"""
    sc, flat_a = S.build("textured")
    ball = [i for i in range(flat_a.n_nodes) if flat_a.node(i).type == abi.ACN_SPHERE and flat_a.node(i).prm[0] == 0.9 and flat_a.node(i).radiance == 0]
    assert len(ball) == 1
    flat_b = rigid_copy(flat_a, ball[0], shift=(0.7, 0.0, 0.0))
    W, H = 96, 72
    pos = A.main_pass_positions(W, H)
    h = A.Handle(flat_a)
    try:
        surf_a = h.surface_positions(pos).raw
        sh_a = h.shadow_records(surf_a, 16)
        stats_a = MM.synthetic_stats(len(pos))
        prm_a = MM.copy_params(h.params)
        h.replace(flat_b)
        surf_b = h.surface_positions(pos).raw
        sh_b = h.shadow_records(surf_b, 16)
        table, report = A.motion_from_scenes(flat_a, flat_b)
        assert report["moved"] == 1
        kinds = abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS & ~abi.ACN_SURF_FRESNEL      # the floor is polished: history on Fresnel surfaces too
        hist, motion = h.reproject_moving(surf_b, prm_a, surf_a, stats_a, table, reject_kinds=kinds)
        want, want_change = SM.limit_history(hist.raw, motion, sh_b, sh_a, W, H)
        got, change = h.shadow_limit_history(hist, motion, sh_b, sh_a, W, H)
        assert_same_bits(got.raw, want)
        assert_same_bits(change, want_change)
        dev, dev_change = guard_dev(h, hist.raw, motion, sh_b, sh_a, W, H)
        assert_same_bits(dev, want)
        assert_same_bits(dev_change, want_change)
        has = ~SM.empty(hist.raw[:, 0])
        limited = has & (got.raw != hist.raw).any(axis=1)
        untouched = has & ~np.isnan(change) & (got.raw == hist.raw).all(axis=1)
        print(f"{int(has.sum())} positions with a history: {int(limited.sum())} limited, {int(untouched.sum())} compared and untouched")
        assert limited.sum() >= 1 and untouched.sum() >= 1
        assert (got.raw[limited, 0] == 1.0).all() and (change[limited] > 0.25).all()
        # the same frame twice, camera and world at rest: change is exactly 0 wherever it is formed, nothing is limited
        rest, motion_rest = h.reproject(surf_b, MM.copy_params(h.params), surf_b, stats_a, reject_kinds=kinds)
        same, change_rest = h.shadow_limit_history(rest, motion_rest, sh_b, sh_b, W, H)
        assert_same_bits(same.raw, rest.raw)
        assert (change_rest[~np.isnan(change_rest)] == 0).all() and (~np.isnan(change_rest)).sum() >= 1000
    finally:
        h.close()


# ---- the tools ----
def test_the_tools_write_the_share_plane_and_run_the_guard(tmp_path, capsys):
    """tools/render_aovs.py --shadow writes plane [ 5 ] of the records; tools/render_turntable.py --temporal --shadow-guard runs the
    guard between reproject and merge and reports it per frame; the options are refused where they do not belong"""
    import os
    import re
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import render_aovs as aovs
    import render_turntable as tool
    flat = MM.two_frames()["prev_flat"]
    scene = tmp_path / "pose.npz"
    flat.save(str(scene))
    aovs.main([str(scene), str(tmp_path / "aov"), "--shadow", "8"])
    share = aovs.read_pfm(tmp_path / "aov" / "shadow.pfm")
    rec = np.load(tmp_path / "aov" / "shadow.npy")
    W, H = int(flat.params.image_width), int(flat.params.image_height)
    assert share.shape == (H, W) and rec.shape == (W * H, 16)
    assert np.array_equal(share.reshape(-1), rec[:, 5].astype(np.float32)) and 0 < (share > 0).mean() and share.max() <= 1
    h = A.Handle(flat)
    try:
        assert np.array_equal(rec, h.shadow_records(h.surface_positions(A.main_pass_positions(W, H)), 8))
    finally:
        h.close()
    capsys.readouterr()
    tool.main([str(scene), str(tmp_path / "t_%d.pnm"), "--frames", "3", "--orbit-deg", "6", "--temporal", "--samples", "2", "--allow-fresnel",
               "--shadow-guard", "--shadow-samples", "8", "--shadow-tolerance", "0.3"])
    said = capsys.readouterr().out
    lim = [float(v) for v in re.findall(r"^frame \d+: [0-9.]+ of the pixels took a history, mean n [0-9.]+, the shadow guard limited ([0-9.]+) of the histories", said, re.M)]
    assert len(lim) == 3 and lim[0] == 0.0 and all(0.0 <= v < 0.2 for v in lim), said
    assert all(open(tmp_path / f"t_{f}.pnm", "rb").read().startswith(b"P6") for f in range(3))
    for bad in (["--shadow-guard"], ["--temporal", "--samples", "2", "--shadow-samples", "8"], ["--temporal", "--samples", "2", "--shadow-guard", "--shadow-samples", "3"],
                ["--temporal", "--samples", "2", "--shadow-guard", "--shadow-tolerance", "-1"], ["--temporal", "--samples", "2", "--shadow-drop"]):
        with pytest.raises(SystemExit):
            tool.main([str(scene), str(tmp_path / "x_%d.pnm"), "--frames", "2", "--orbit-deg", "6"] + bad)
    with pytest.raises(SystemExit):
        aovs.main([str(scene), str(tmp_path / "aov2"), "--shadow", "5"])

"""Layered records merged across passes and resolved on the GPU (acn_lens_layers_merge*, acn_lens_layers_resolve_dev;
include/actinon_hip.h) against the numpy model of tests/lens_layers_merge_model.py, bit for bit (test_lens_layers_merge_cpu.py checks
the model against answers known without it); a progressive sequence end to end; tools/render_progressive.py --layers; the calls'
contracts: streams, indices, refusals, the renderer left alone.  Bit for bit means Y.same_bits: which NaN a NaN result is, the header
leaves open."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import lens_layers_merge_model as G
import lens_layers_model as Y
import scenes_util as S
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = dict(aperture=0.15, focus=12.0, jitter=True)                           # the lens of tests/test_gpu_lens_surface.py
W, H, K = 96, 54, 4
THRESHOLD = 0.1                                                               # the noise above which the third pass samples again
# sha256 of the file `render_progressive.py SCENE OUT --samples 4 --passes 3 --target-noise 0.1 --denoise --select library --aperture 0.15
# --focus 12` writes for wine_glass_c2 96 x 54, taken on the commit before --layers existed
PLAIN_SHA256 = "4b9c3acfa8359dc10f88e1a67e176cffa05f9a06fb90207cc2399c9e38035739"


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want):
    bad = Y.same_bits(got, want)
    got, want = np.asarray(got), np.asarray(want)
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


def planes(records):
    return np.stack([r.raw for r in records])


def merge_dev(h, a_surf, a_st, b_surf, b_st, index=None):
    """the _dev form on torch buffers with a NaN record behind every buffer -> ( surf, st ) read back"""
    import torch
    n_acc, n_part = a_st.shape[1], b_st.shape[1]
    up = lambda a, stride: torch.cat([torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, stride),
                                      torch.full((1, stride), float("nan"), dtype=torch.float64)]).to("cuda")
    d_as, d_at, d_bs, d_bt = up(a_surf, 16), up(a_st, 8), up(b_surf, 16), up(b_st, 8)
    d_idx = None if index is None else torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).to("cuda")
    torch.cuda.synchronize()
    h.lens_layers_merge_dev(d_as.data_ptr(), d_at.data_ptr(), n_acc, d_bs.data_ptr(), d_bt.data_ptr(), n_part, None if d_idx is None else d_idx.data_ptr())
    surf, st = d_as.cpu().numpy(), d_at.cpu().numpy()
    assert np.isnan(surf[-1]).all() and np.isnan(st[-1]).all()
    assert_same_bits(d_bs.cpu().numpy()[:-1].reshape(b_surf.shape), b_surf)   # the part stays
    assert_same_bits(d_bt.cpu().numpy()[:-1].reshape(b_st.shape), b_st)
    return surf[:-1].reshape(2, n_acc, 16), st[:-1].reshape(3, n_acc, 8)


def strided(n_acc):
    """the index list of the tests: every third position, with a -1 and an n_acc among them (behind them where the list is short)"""
    idx = np.arange(0, n_acc, 3, dtype=np.int64)
    if len(idx) >= 3:
        idx[1], idx[-1] = -1, n_acc
        return idx
    return np.concatenate([idx, np.array([-1, n_acc], dtype=np.int64)])


# ---- the merge against the model ----
@pytest.mark.parametrize("n_acc", [1, 63, 64, 65, 257, 1000])
def test_merge_against_the_model(h, detmath_cpu, n_acc):
    """position i is hand-made pattern i % P: every pattern meets every lane of a wave and the last, partial workgroup.  A null index
    through the host form; a strided index with a -1 and an n_acc through the _dev form, the untouched positions keeping their bytes"""
    a_surf, a_st, b_surf, b_st = G.tiled(n_acc)
    want_surf, want_st = G.merge(detmath_cpu, a_surf, a_st, b_surf, b_st)
    surf, st = h.lens_layers_merge(a_surf, a_st, b_surf, b_st)
    assert_same_bits(planes(surf), want_surf)
    assert_same_bits(planes(st), want_st)
    got_surf, got_st = merge_dev(h, a_surf, a_st, b_surf, b_st)
    assert_same_bits(got_surf, want_surf)
    assert_same_bits(got_st, want_st)
    idx = strided(n_acc)
    target = np.clip(idx, 0, n_acc - 1)
    p_surf, p_st = np.ascontiguousarray(b_surf[:, target]), np.ascontiguousarray(b_st[:, target])   # the part of the position it goes to
    want_surf, want_st = G.merge(detmath_cpu, a_surf, a_st, p_surf, p_st, index=idx)
    got_surf, got_st = merge_dev(h, a_surf, a_st, p_surf, p_st, index=idx)
    assert_same_bits(got_surf, want_surf)
    assert_same_bits(got_st, want_st)
    untouched = np.ones(n_acc, bool)
    untouched[idx[(idx >= 0) & (idx < n_acc)]] = False
    assert (bits(got_surf[:, untouched]) == bits(a_surf[:, untouched])).all() and (bits(got_st[:, untouched]) == bits(a_st[:, untouched])).all()
    if n_acc >= 3:
        assert untouched.sum() >= n_acc // 2 and (-1 in idx) and (n_acc in idx)


def test_the_host_form_refuses_bad_indices(h):
    a_surf, a_st, b_surf, b_st = G.tiled(8)
    for idx, word in (([0, 1, 2, 8], "out of range"), ([0, -1, 2, 3], "out of range"), ([0, 1, 2, 1], "duplicate")):
        acc_s, acc_t = a_surf.copy(), a_st.copy()
        i = np.array(idx, dtype=np.int64)
        o = h._plain_opts(False, None)
        st = hip.acn_lens_layers_merge(h.h, acc_s.ctypes.data, acc_t.ctypes.data, 8, np.ascontiguousarray(b_surf[:, :4]).ctypes.data,
                                       np.ascontiguousarray(b_st[:, :4]).ctypes.data, 4, i.ctypes.data, C.byref(o))
        assert st == abi.ACN_ERR_ARG and word in hip.acn_last_error().decode()
        assert (bits(acc_s) == bits(a_surf)).all() and (bits(acc_t) == bits(a_st)).all()


def test_merge_on_a_callers_stream(h, detmath_cpu):
    """behind a kernel that fills the part on that stream; the call does not synchronise: the result is right only if it ran in
    stream order"""
    import torch
    n = 257
    a_surf, a_st, b_surf, b_st = G.tiled(n)
    idx = strided(n)
    target = np.clip(idx, 0, n - 1)
    p_surf, p_st = np.ascontiguousarray(b_surf[:, target]), np.ascontiguousarray(b_st[:, target])
    want_surf, want_st = G.merge(detmath_cpu, a_surf, a_st, p_surf, p_st, index=idx)
    src_s, src_t = torch.from_numpy(p_surf).to("cuda"), torch.from_numpy(p_st).to("cuda")
    d_as, d_at = torch.from_numpy(a_surf).to("cuda"), torch.from_numpy(a_st).to("cuda")
    d_idx = torch.from_numpy(idx).to("cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_bs, d_bt = torch.zeros_like(src_s), torch.zeros_like(src_t)
        d_bs.copy_(src_s); d_bt.copy_(src_t)                                  # kernels on s: the part is not there before them
        h.lens_layers_merge_dev(d_as.data_ptr(), d_at.data_ptr(), n, d_bs.data_ptr(), d_bt.data_ptr(), len(idx), d_idx.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert_same_bits(d_as.cpu().numpy(), want_surf)
    assert_same_bits(d_at.cpu().numpy(), want_st)


def test_a_position_does_not_depend_on_its_neighbours(h):
    n = 130
    a_surf, a_st, b_surf, b_st = G.tiled(n)
    surf, st = merge_dev(h, a_surf, a_st, b_surf, b_st)
    sel = np.array([0, 7, 63, 64, 129])
    cut = lambda a: np.ascontiguousarray(a[:, sel])
    few_surf, few_st = merge_dev(h, cut(a_surf), cut(a_st), cut(b_surf), cut(b_st))
    assert_same_bits(few_surf, surf[:, sel])
    assert_same_bits(few_st, st[:, sel])
    for i in (7, 64):
        one_surf, one_st = merge_dev(h, a_surf[:, i:i + 1], a_st[:, i:i + 1], b_surf[:, i:i + 1], b_st[:, i:i + 1])
        assert_same_bits(one_surf, surf[:, i:i + 1])
        assert_same_bits(one_st, st[:, i:i + 1])
    perm = np.random.default_rng(1).permutation(n)
    p_surf, p_st = merge_dev(h, a_surf[:, perm], a_st[:, perm], b_surf[:, perm], b_st[:, perm])
    assert_same_bits(p_surf, surf[:, perm])
    assert_same_bits(p_st, st[:, perm])


# ---- the resolve against the model ----
def test_resolve_against_the_model(h, detmath_cpu, flat):
    """colour saturated and linear, noise, pooled record; an all-EMPTY position, a position of one sample, a rest alone"""
    import torch
    a_surf, a_st, b_surf, b_st = G.tiled(130)
    _, st = G.merge(detmath_cpu, a_surf, a_st, b_surf, b_st)
    st = np.ascontiguousarray(st[:, :70])
    rng = np.random.default_rng(4)
    st[:, 3] = 0.0                                                            # all EMPTY
    st[:, 4] = 0.0; st[0, 4] = G.slot(rng, G.A_, 1)[1]                        # one sample
    st[:, 5] = 0.0; st[2, 5] = G.slot(rng, G.A_, 3)[1]                        # a rest alone
    st[:, 6] = 0.0; st[0, 6, 0] = np.nan; st[1, 6, 0] = 0.5; st[2, 6, 0] = np.inf   # EMPTY, not zeros
    bg, gamma = np.array(flat.params.background_color[:]), float(flat.params.gamma)
    for linear in (False, True):
        want_rgb, want_noise, want_pooled = G.layers_resolve(detmath_cpu, st, bg, gamma, linear)
        rgb, noise, pooled = h.lens_layers_resolve(st, linear=linear)
        assert_same_bits(rgb, want_rgb)
        assert_same_bits(noise, want_noise)
        assert_same_bits(pooled.raw, want_pooled)
    assert noise[3] == np.inf and noise[4] == np.inf and noise[6] == np.inf and np.isfinite(noise[5])
    assert (bits(pooled.raw[[3, 6]]) == 0).all()
    assert_same_bits(h.lens_layers_resolve(st, linear=True)[0][[3, 6]], np.stack([bg] * 2))
    # the noise alone, on a caller's stream; the other outputs null
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.from_numpy(st).to("cuda")
        d_noise = torch.full((71,), float("nan"), dtype=torch.float64, device="cuda")
        h.lens_layers_resolve_dev(d.data_ptr(), 70, None, d_noise.data_ptr(), None, stream=s.cuda_stream)
    s.synchronize()
    assert_same_bits(d_noise.cpu().numpy()[:70], want_noise)
    assert np.isnan(d_noise.cpu().numpy()[70])


# ---- end to end: two full passes, a selection, a third pass by index ----
def progressive(flat):
    """on a fresh handle: passes of K = 4 with seeds 0 and 1 over the raster merged into a zero-filled accumulator, the noise of the
    pooled records, acn_select_above_dev above THRESHOLD, a third pass with seed 2 on the selected pixels merged by index -- all on
    the device.  -> the three passes' planes, the index list and the accumulator after the second and the third merge, read back"""
    import torch
    n = W * H
    hd = A.Handle(flat)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    d_surf, d_st, d_noise = new(2, n, 16), new(3, n, 8), new(n)
    d_idx, d_pos = torch.zeros((n,), dtype=torch.int64, device="cuda"), new(n, 2)
    torch.cuda.synchronize()
    out = {"parts": []}
    for seed in (0, 1):
        d_ps, d_pt = new(2, n, 16), new(3, n, 8)
        torch.cuda.synchronize()
        hd.render_lens_layers_main_pass_dev(0, n, None, d_ps.data_ptr(), d_pt.data_ptr(), follow=True, linear=True, samples=K, seed=seed, **LENS)
        hd.lens_layers_merge_dev(d_surf.data_ptr(), d_st.data_ptr(), n, d_ps.data_ptr(), d_pt.data_ptr(), n)
        out["parts"].append((d_ps.cpu().numpy(), d_pt.cpu().numpy()))
        if seed == 0:
            out["first"] = (d_surf.cpu().numpy(), d_st.cpu().numpy())
    out["second"] = (d_surf.cpu().numpy(), d_st.cpu().numpy())
    hd.lens_layers_resolve_dev(d_st.data_ptr(), n, None, d_noise.data_ptr(), None, linear=True)
    m = hd.select_above_dev(d_noise.data_ptr(), n, THRESHOLD, n, d_index_ptr=d_idx.data_ptr(), d_pos_ptr=d_pos.data_ptr(), raster_width=W)
    out["noise"], out["index"] = d_noise.cpu().numpy(), d_idx.cpu().numpy()[:m]
    d_ps, d_pt = new(2, m, 16), new(3, m, 8)
    torch.cuda.synchronize()
    hd.render_lens_layers_dev(d_pos.data_ptr(), m, None, d_ps.data_ptr(), d_pt.data_ptr(), follow=True, linear=True, samples=K, seed=2, **LENS)
    hd.lens_layers_merge_dev(d_surf.data_ptr(), d_st.data_ptr(), n, d_ps.data_ptr(), d_pt.data_ptr(), m, d_idx.data_ptr())
    out["parts"].append((d_ps.cpu().numpy(), d_pt.cpu().numpy()))
    out["third"] = (d_surf.cpu().numpy(), d_st.cpu().numpy())
    hd.close()
    return out


@pytest.fixture(scope="module")
def sequence(flat):
    return progressive(flat)


def test_the_sequence_against_the_model(detmath_cpu, flat, sequence):
    parts, idx = sequence["parts"], sequence["index"]
    n = W * H
    assert 0 < len(idx) < n and (np.diff(idx) > 0).all()
    for l in range(2):                                                        # a zero-filled accumulator becomes the first pass
        assert_same_bits(sequence["first"][l], parts[0][l])
    second = G.merge(detmath_cpu, parts[0][0], parts[0][1], parts[1][0], parts[1][1])
    assert_same_bits(sequence["second"][0], second[0])
    assert_same_bits(sequence["second"][1], second[1])
    assert (second[1][1][:, 0] >= 1).any(), "no pixel with a layer 1 at this aperture"   # (0.15 suffices: 169 of the 5184 pixels after the third merge)
    bg, gamma = np.array(flat.params.background_color[:]), float(flat.params.gamma)
    noise = G.layers_resolve(detmath_cpu, second[1], bg, gamma, True)[1]
    assert_same_bits(sequence["noise"], noise)
    assert np.array_equal(idx, np.flatnonzero(noise > THRESHOLD))
    third = G.merge(detmath_cpu, second[0], second[1], parts[2][0], parts[2][1], index=idx)
    assert_same_bits(sequence["third"][0], third[0])
    assert_same_bits(sequence["third"][1], third[1])
    cnt = sequence["third"][1][:, :, 0].sum(axis=0)
    want = np.full(n, 2.0 * K); want[idx] += K
    assert (cnt == want).all()                                                # every sample is in exactly one of the three records


def test_the_sequence_repeats_bit_for_bit(flat, sequence):
    again = progressive(flat)
    assert np.array_equal(again["index"], sequence["index"])
    for key in ("second", "third"):
        for l in range(2):
            assert_same_bits(again[key][l], sequence[key][l])


def test_the_layered_filter_takes_the_merged_planes(flat, sequence):
    """Gate, that of test_gpu_lens_surface.py ("below raw"): over the pixels filterable in plane 0 the linear MSE of acn_denoise_layers
    of the merged planes against a K = 256, seed 9 frame is below that of the unfiltered resolve of the same planes.
    Seen on an MI355X, 5137 pixels: pooled mean 4.888e-3, layered filter 3.500e-3 (0.716 of it); 169 pixels with a layer 1, 82 with a rest."""
    import torch
    surf, st = sequence["third"]
    n = W * H
    hd = A.Handle(flat)
    pos = S.positions(flat)
    ref = hd.render_lens(pos, linear=True, **dict(LENS, samples=256, seed=9)).reshape(H, W, 3)
    raw = hd.lens_layers_resolve(st, linear=True)[0].reshape(H, W, 3)
    d_st, d_surf = torch.from_numpy(st).to("cuda"), torch.from_numpy(surf).to("cuda")
    d_out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hd.denoise_layers_dev(d_st.data_ptr(), d_surf.data_ptr(), W, H, d_out.data_ptr())
    out = d_out.cpu().numpy().reshape(H, W, 3)
    hd.close()
    with np.errstate(all="ignore"):
        ok = (D.filterable(surf[0], st[0][:, 1:4] / D.albedo(surf[0])) & ~T.empty(st[0])).reshape(H, W)
    assert ok.mean() > 0.5
    mse = lambda x: float(np.mean((x[ok] - ref[ok]) ** 2))
    print(f"wine_glass_c2 96x54, 2 full passes of K=4 and a third on {len(sequence['index'])} pixels, merged, vs K=256: linear mse over "
          f"{int(ok.sum())} pixels filterable in plane 0: raw {mse(raw):.4e}  layered filter {mse(out):.4e} ({mse(out) / mse(raw):.3f} of raw); "
          f"{int((st[1][:, 0] >= 1).sum())} pixels with a layer 1, {int((st[2][:, 0] >= 1).sum())} with a rest")
    assert mse(out) < mse(raw), (mse(out), mse(raw))


# ---- the tool ----
def test_the_progressive_tool_with_layers(tmp_path, flat):
    """--layers --denoise --select library writes an image; without --layers the command writes the bytes it wrote before the option
    existed"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_progressive as tool
    scene = tmp_path / "scene.npz"
    flat.save(str(scene))
    base = [str(scene), None, "--samples", "4", "--passes", "3", "--target-noise", "0.1", "--denoise", "--select", "library",
            "--aperture", "0.15", "--focus", "12"]
    data = {}
    for key, extra in (("plain", []), ("layers", ["--layers"]), ("layers, torch", ["--layers", "--select", "torch"])):
        args = list(base)
        args[1] = str(tmp_path / (key.replace(", ", "_") + ".pnm"))
        tool.main(args + extra)
        data[key] = open(args[1], "rb").read()
    assert hashlib.sha256(data["plain"]).hexdigest() == PLAIN_SHA256
    assert data["layers"].startswith(b"P6") and len(data["layers"]) == len(data["plain"]) and data["layers"] != data["plain"]
    assert data["layers, torch"] == data["layers"]                            # both --select modes take the same pixels
    with pytest.raises(SystemExit):
        tool.parse_args(base[:1] + ["x.pnm"] + base[2:] + ["--layers", "--guides", "lens"])


# ---- isolation ----
def test_the_calls_leave_the_renderer_alone(flat):
    pos = S.positions(flat)[::7]
    hd = A.Handle(flat)
    hd.render_positions(pos, linear=True)                                   # a warm handle
    before = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    raw = (C.c_double * 25)()
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    raw_before = list(raw)
    counters = hd.last_counters_raw(10)
    kernel_ms = hd.last_kernel_ms()
    a_surf, a_st, b_surf, b_st = G.tiled(130)
    surf, st = hd.lens_layers_merge(a_surf, a_st, b_surf, b_st)
    resolved = hd.lens_layers_resolve(planes(st))
    assert hip.acn_last_stage_ms(hd.h, raw, 25) == abi.ACN_OK
    assert list(raw) == raw_before                                          # [ 23 ], [ 24 ] included: nothing of the workspace moved
    assert list(hd.last_counters_raw(10)) == list(counters) and hd.last_kernel_ms() == kernel_ms
    after = hd.render_positions(pos, linear=True)
    assert hd.last_stages()["retries"] == 0
    assert np.array_equal(before, after)
    assert_same_bits(planes(hd.lens_layers_merge(a_surf, a_st, b_surf, b_st)[1]), planes(st))
    assert_same_bits(hd.lens_layers_resolve(planes(st))[1], resolved[1])
    hd.close()


# ---- errors ----
def test_refusals_leave_the_output_untouched(flat):
    """Every ACN_ERR_ARG of the two calls: the status, acn_last_error, and not one word written, on host and device buffers; then the
    handle still works"""
    import torch
    n = 40
    h = A.Handle(flat)
    o = h._plain_opts(False, None)
    a_surf, a_st, b_surf, b_st = G.tiled(n)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    d_as, d_at, d_rgb, d_noise, d_pooled = nan(2 * n, 16), nan(3 * n, 8), nan(n, 3), nan(n), nan(n, 8)
    d_bs, d_bt = torch.from_numpy(b_surf).to("cuda"), torch.from_numpy(b_st).to("cuda")
    d_idx = torch.arange(n, dtype=torch.int64, device="cuda")
    h_as, h_at = np.full((2 * n, 16), np.nan), np.full((3 * n, 8), np.nan)
    idx = np.arange(n, dtype=np.int64)
    torch.cuda.synchronize()

    def refused(table, word):
        for name, call in table.items():
            hip.acn_render_positions(None, None, 0, None, None)            # (sets another message)
            assert call() == abi.ACN_ERR_ARG, name
            msg = hip.acn_last_error().decode()
            assert msg and word in msg, (name, msg)
            torch.cuda.synchronize()
            assert np.isnan(h_as).all() and np.isnan(h_at).all(), name
            assert all(bool(torch.isnan(a).all()) for a in (d_as, d_at, d_rgb, d_noise, d_pooled)), name

    def calls(handle, opts, n_acc=n, n_part=n, das=d_as.data_ptr(), dat=d_at.data_ptr(), dbs=d_bs.data_ptr(), dbt=d_bt.data_ptr(), di=d_idx.data_ptr(),
              has=h_as.ctypes.data, hat=h_at.ctypes.data, hbs=b_surf.ctypes.data, hbt=b_st.ctypes.data, hi=idx.ctypes.data):
        return {"merge": lambda: hip.acn_lens_layers_merge(handle, has, hat, n_acc, hbs, hbt, n_part, hi, C.byref(opts)),
                "merge_dev": lambda: hip.acn_lens_layers_merge_dev(handle, das, dat, n_acc, dbs, dbt, n_part, di, C.byref(opts))}

    def resolve(handle, opts, ds=d_bt.data_ptr(), rgb=d_rgb.data_ptr(), noise=d_noise.data_ptr(), pooled=d_pooled.data_ptr()):
        return {"resolve": lambda: hip.acn_lens_layers_resolve_dev(handle, ds, n, rgb, noise, pooled, C.byref(opts))}

    only = lambda table, *names: {k: v for k, v in table.items() if k in names}
    refused(calls(None, o), "handle")
    refused(resolve(None, o), "handle")
    for kw in ("has", "hat", "hbs", "hbt"):
        refused(only(calls(h.h, o, **{kw: None}), "merge"), "null")
    for kw in ("das", "dat", "dbs", "dbt"):
        refused(only(calls(h.h, o, **{kw: None}), "merge_dev"), "null")
    refused(resolve(h.h, o, ds=None), "null")
    world2 = h._plain_opts(False, None)
    world2.shard_world = 2
    refused(calls(h.h, world2), "sharded")
    refused(resolve(h.h, world2), "sharded")
    for kw, buf in (("das", d_as), ("dat", d_at), ("dbs", d_bs), ("dbt", d_bt)):
        refused(only(calls(h.h, o, **{kw: buf.data_ptr() + 8}), "merge_dev"), "align")
    refused(only(calls(h.h, o, di=d_idx.data_ptr() + 4), "merge_dev"), "int64_t")
    refused(only(calls(h.h, o, has=h_as.ctypes.data + 8), "merge"), "align")
    refused(resolve(h.h, o, ds=d_bt.data_ptr() + 8), "align")
    refused(resolve(h.h, o, pooled=d_pooled.data_ptr() + 8), "align")
    refused(resolve(h.h, o, noise=d_noise.data_ptr() + 4), "align")
    # a null index needs n_part <= n_acc; the host form reads its list
    refused(calls(h.h, o, n_acc=n - 1, di=None, hi=None), "n_part <= n_acc")
    bad = idx.copy(); bad[5] = n
    refused(only(calls(h.h, o, hi=bad.ctypes.data), "merge"), "out of range")
    twice = idx.copy(); twice[5] = 4
    refused(only(calls(h.h, o, hi=twice.ctypes.data), "merge"), "duplicate")
    # nothing to do is ACN_OK and writes nothing, null buffers included
    for call in (lambda: hip.acn_lens_layers_merge_dev(h.h, d_as.data_ptr(), d_at.data_ptr(), n, None, None, 0, None, C.byref(o)),
                 lambda: hip.acn_lens_layers_merge(h.h, h_as.ctypes.data, h_at.ctypes.data, n, None, None, 0, None, None),
                 lambda: hip.acn_lens_layers_merge_dev(h.h, None, None, 0, d_bs.data_ptr(), d_bt.data_ptr(), n, d_idx.data_ptr(), C.byref(o)),
                 lambda: hip.acn_lens_layers_resolve_dev(h.h, None, 0, d_rgb.data_ptr(), d_noise.data_ptr(), d_pooled.data_ptr(), C.byref(o)),
                 lambda: hip.acn_lens_layers_resolve_dev(h.h, d_bt.data_ptr(), n, None, None, None, C.byref(o))):
        assert call() == abi.ACN_OK
    torch.cuda.synchronize()
    assert np.isnan(h_as).all() and np.isnan(h_at).all() and all(bool(torch.isnan(a).all()) for a in (d_as, d_at, d_rgb, d_noise, d_pooled))
    # and the handle works
    got_surf, got_st = h.lens_layers_merge(a_surf, a_st, b_surf, b_st)
    assert planes(got_st).shape == (3, n, 8)
    h.close()

"""acn_fill_stats on the GPU against the numpy model of tests/fill_model.py, bit for bit in both outputs (include/actinon_hip.h,
"Filling", states every expression and its order; test_fill_cpu.py checks the model's properties), the call's contract (streams,
device buffers, refusals, the renderer left alone), the workflow the header describes -- fill, select by need, render, merge into
the sparse accumulator, fill again, filter -- what the fill buys against a converged frame, and tools/render_preview.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import fill_model as F
import scenes_util as S
import stats_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23
PARAMS = {"defaults": dict(), "radius1": dict(radius=1), "radius8_power0": dict(radius=8, normal_power_log2=0),
          "no_demodulate": dict(demodulate=False)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"


@pytest.fixture(scope="module")
def flat():
    return S.build("wine_glass_c2")[1]


@pytest.fixture(scope="module")
def h(flat):
    """the fill takes of the scene its background colour alone"""
    handle = A.Handle(flat)
    yield handle
    handle.close()


@pytest.fixture(scope="module")
def bg(flat):
    return np.array(flat.params.background_color[:])


def assert_same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:5], [got[tuple(i)] for i in bad[:5]], [want[tuple(i)] for i in bad[:5]])


@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("lattice", [2, 4])
@pytest.mark.parametrize("shape", [(W, H), (1, 64), (64, 1), (5, 5), (17, 16), (33, 3)])
def test_synthetic_frames_have_the_models_bits(h, bg, detmath_cpu, shape, lattice, params):
    w, hh = shape
    stats, rec = F.synthetic_sparse(w, hh, lattice)
    got, need = h.fill_stats(stats, rec, w, hh, **PARAMS[params])
    want, want_need = F.fill(detmath_cpu, stats, rec, w, hh, bg, **PARAMS[params])
    assert need.shape == (hh, w)
    assert_same_bits(got.raw, want)
    assert_same_bits(need, want_need)


def test_results_do_not_depend_on_wave_neighbours(h):
    """the frame inside a larger one whose other pixels are misses: other tiles, other waves, the same bits"""
    stats, rec = F.synthetic_sparse(W, H, 2)
    plain, plain_need = h.fill_stats(stats, rec, W, H)
    assert (plain_need > 0).any() and np.isinf(plain_need).any()
    for (bw, bh, x0, y0) in ((W + 30, H + 19, 19, 9), (W + 1, H + 1, 1, 0), (W + 64, H, 64, 0)):
        big_stats = np.zeros((bh, bw, 8))
        big_rec = D.blank(bh * bw).reshape(bh, bw, 16)
        big_stats[y0:y0 + H, x0:x0 + W] = stats.reshape(H, W, 8)
        big_rec[y0:y0 + H, x0:x0 + W] = rec.reshape(H, W, 16)
        got, need = h.fill_stats(big_stats.reshape(-1, 8), big_rec.reshape(-1, 16), bw, bh)
        assert_same_bits(got.raw.reshape(bh, bw, 8)[y0:y0 + H, x0:x0 + W], plain.raw.reshape(H, W, 8))
        assert_same_bits(need[y0:y0 + H, x0:x0 + W], plain_need)
        outside = np.ones((bh, bw), bool)
        outside[y0:y0 + H, x0:x0 + W] = False
        assert (need[outside] == 0.0).all() and (got.raw.reshape(bh, bw, 8)[outside][:, 0] == 1.0).all()   # misses: BACKGROUND


def test_device_buffers_a_callers_stream_and_a_null_need(h, bg, detmath_cpu):
    import torch
    n = W * H
    stats, rec = F.synthetic_sparse(W, H, 2)
    for params in (dict(), dict(radius=5, sigma_px=2.5, sigma_plane=0.3)):
        want, want_need = F.fill(detmath_cpu, stats, rec, W, H, bg, **params)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_stats = torch.from_numpy(stats.copy()).to("cuda")
            d_rec = torch.from_numpy(rec.copy()).to("cuda")
            d_out = torch.full((n + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
            d_need = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
            d_only = torch.full((n + 1, 8), float("nan"), dtype=torch.float64, device="cuda")
            h.fill_stats_dev(d_stats.data_ptr(), d_rec.data_ptr(), W, H, d_out.data_ptr(), d_need.data_ptr(), stream=s.cuda_stream, **params)
            h.fill_stats_dev(d_stats.data_ptr(), d_rec.data_ptr(), W, H, d_only.data_ptr(), None, stream=s.cuda_stream, **params)
        s.synchronize()
        out, need, only = d_out.cpu().numpy(), d_need.cpu().numpy(), d_only.cpu().numpy()
        assert_same_bits(out[:n], want)
        assert_same_bits(need[:n].reshape(H, W), want_need)
        assert_same_bits(only[:n], want)                                        # out_need null: the records alone
        assert np.isnan(out[n]).all() and np.isnan(need[n]) and np.isnan(only[n]).all()   # nothing behind either output
        assert_same_bits(d_stats.cpu().numpy(), stats)                          # the input stays
        assert_same_bits(d_rec.cpu().numpy(), rec)
        d_sync = torch.empty((n, 8), dtype=torch.float64, device="cuda")
        d_sync_need = torch.empty((n,), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h.fill_stats_dev(d_stats.data_ptr(), d_rec.data_ptr(), W, H, d_sync.data_ptr(), d_sync_need.data_ptr(), **params)   # the handle's stream: the call waits
        assert_same_bits(d_sync.cpu().numpy(), want)
        assert_same_bits(d_sync_need.cpu().numpy().reshape(H, W), want_need)


def test_refusals_leave_the_outputs_untouched(h):
    import torch
    n = W * H
    stats, rec = F.synthetic_sparse(W, H, 2)
    d_stats = torch.from_numpy(stats.copy()).to("cuda")
    d_rec = torch.from_numpy(rec.copy()).to("cuda")
    d_out = torch.full((n + 1, 8), 7.25, dtype=torch.float64, device="cuda")
    d_need = torch.full((n + 1,), 7.25, dtype=torch.float64, device="cuda")
    d_both = torch.cat([d_stats, torch.full((n, 8), 7.25, dtype=torch.float64, device="cuda")])     # stats, then room behind it
    torch.cuda.synchronize()
    st, rc, out, need = d_stats.data_ptr(), d_rec.data_ptr(), d_out.data_ptr(), d_need.data_ptr()
    cases = [
        ("radius", lambda: h.fill_stats_dev(st, rc, W, H, out, need, radius=9)),
        ("normal_power_log2", lambda: h.fill_stats_dev(st, rc, W, H, out, need, normal_power_log2=11)),
        ("sigma", lambda: h.fill_stats_dev(st, rc, W, H, out, need, sigma_px=-1.0)),
        ("sigma", lambda: h.fill_stats_dev(st, rc, W, H, out, need, sigma_plane=float("nan"))),
        ("sigma", lambda: h.fill_stats_dev(st, rc, W, H, out, need, sigma_px=float("inf"))),
        ("width", lambda: h.fill_stats_dev(st, rc, 0, H, out, need)),
        ("null", lambda: h.fill_stats_dev(st, rc, W, H, None, need)),
        ("null", lambda: h.fill_stats_dev(None, rc, W, H, out, need)),
        ("align", lambda: h.fill_stats_dev(st + 8, rc, W, H - 1, out, need)),
        ("align", lambda: h.fill_stats_dev(st, rc + 8, W, H - 1, out, need)),
        ("align", lambda: h.fill_stats_dev(st, rc, W, H - 1, out + 8, need)),
        ("align", lambda: h.fill_stats_dev(st, rc, W, H, out, need + 4)),
        ("overlaps", lambda: h.fill_stats_dev(d_both.data_ptr(), rc, W, H, d_both.data_ptr(), need)),                # in place
        ("overlaps", lambda: h.fill_stats_dev(d_both.data_ptr(), rc, W, H, d_both.data_ptr() + 64 * (n - 1), need)),   # the last record
        ("overlaps", lambda: h.fill_stats_dev(st, rc, W, H, out, out + 64)),                                            # need inside out_stats
    ]
    for word, call in cases:
        with pytest.raises(A.AcnError) as e:
            call()
        assert e.value.status == A.abi.ACN_ERR_ARG and word in str(e.value), (word, str(e.value))
    p = A.abi.FillParams()
    p.struct_size, p.flags = 32, 4
    for size, flags in ((32, 4), (3, 0)):
        p.struct_size, p.flags = size, flags
        assert A.hip.acn_fill_stats_dev(h.h, st, rc, W, H, p, out, need, None) == A.abi.ACN_ERR_ARG
    o = h._plain_opts(False, None)
    o.shard_world = 2
    assert A.hip.acn_fill_stats_dev(h.h, st, rc, W, H, None, out, need, o) == A.abi.ACN_ERR_ARG
    assert A.hip.acn_fill_stats_dev(None, st, rc, W, H, None, out, need, None) == A.abi.ACN_ERR_ARG
    torch.cuda.synchronize()
    assert (d_out == 7.25).all() and (d_need == 7.25).all() and (d_both[n:] == 7.25).all()
    assert_same_bits(d_both[:n].cpu().numpy(), stats)
    # the host form refuses the same, and a buffer right behind the input is no overlap
    host_out, host_need = np.full((n, 8), 7.25), np.full((H, W), 7.25)
    with pytest.raises(A.AcnError) as e:
        h.fill_stats(stats, rec, W, H, radius=9)
    assert e.value.status == A.abi.ACN_ERR_ARG
    assert A.hip.acn_fill_stats(h.h, stats.ctypes.data, rec.ctypes.data, W, H, None, stats.ctypes.data, host_need.ctypes.data, None) == A.abi.ACN_ERR_ARG
    assert (host_out == 7.25).all() and (host_need == 7.25).all()
    h.fill_stats_dev(d_both.data_ptr(), rc, W, H, d_both.data_ptr() + 64 * n, need)
    torch.cuda.synchronize()
    assert_same_bits(d_both[n:].cpu().numpy(), h.fill_stats(stats, rec, W, H)[0].raw)


def test_a_fill_call_leaves_the_renderer_alone():
    sc, flat = S.build("wine_glass_c2")
    pos = S.positions(flat)
    stats, rec = F.synthetic_sparse(96, 54, 2)
    hd = A.Handle(flat)
    before = hd.render_positions(pos, linear=True)
    st0 = hd.last_stages()
    first, first_need = hd.fill_stats(stats, rec, 96, 54)
    big, _ = hd.fill_stats(np.tile(stats.reshape(54, 96, 8), (3, 2, 1)).reshape(-1, 8), np.tile(rec.reshape(54, 96, 16), (3, 2, 1)).reshape(-1, 16),
                           192, 162)                                                                  # the scratch grows
    again, again_need = hd.fill_stats(stats, rec, 96, 54)
    after = hd.render_positions(pos, linear=True)
    st1 = hd.last_stages()
    hd.close()
    assert len(big) == 162 * 192
    assert_same_bits(first.raw, again.raw)
    assert_same_bits(first_need, again_need)
    assert np.array_equal(before, after)
    assert st1["retries"] == 0
    assert st1["workspace_bytes"] == st0["workspace_bytes"] and st1["workspace_allocs"] == st0["workspace_allocs"], (st0, st1)


def lattice_index(w, hh, lattice):
    ys, xs = np.mgrid[0:hh:lattice, 0:w:lattice]
    return (ys * w + xs).reshape(-1).astype(np.int64)


def test_the_workflow_composes(detmath_cpu):
    """wine_glass 96 x 54, K = 4, lattice 2: sparse pass, fill, select above 0.5, render, merge into the SPARSE accumulator, fill again,
    filter the filled frame"""
    w, hh, K = 96, 54, 4
    sc = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=8, direct_samples=16)
    flat = sc.flatten()
    bg = np.array(flat.params.background_color[:])
    pos = S.positions(flat)
    n = w * hh
    hd = A.Handle(flat)
    rec = hd.surface_positions(pos, follow=True).raw
    idx = lattice_index(w, hh, 2)
    _, part = hd.render_lens_stats(pos[idx], linear=True, samples=K, jitter=True, seed=0)
    acc = hd.lens_stats_merge(np.zeros((n, 8)), part, idx)
    filled, need = hd.fill_stats(acc, rec, w, hh)
    want, want_need = F.fill(detmath_cpu, acc.raw, rec, w, hh, bg)
    assert_same_bits(filled.raw, want)
    assert_same_bits(need, want_need)
    sel, sel_pos, count = hd.select_above(need.reshape(-1), 0.5, raster_width=w)
    assert count == len(sel) and 0 < count < n - len(idx)
    assert np.array_equal(sel, np.flatnonzero(want_need.reshape(-1) > 0.5)) and np.array_equal(sel_pos, pos[sel])
    assert SM.empty(acc.raw[sel]).all()                                            # no rendered position is selected
    _, part2 = hd.render_lens_stats(sel_pos, linear=True, samples=K, jitter=True, seed=1)
    acc2 = hd.lens_stats_merge(acc, part2, sel)
    assert_same_bits(acc2.raw[sel], part2.raw)                                     # an EMPTY record takes the part bit for bit
    filled2, need2 = hd.fill_stats(acc2, rec, w, hh)
    assert_same_bits(filled2.raw[sel], part2.raw)                                  # now RENDERED
    assert (need2.reshape(-1)[sel] == -1.0).all()
    want2, want_need2 = F.fill(detmath_cpu, acc2.raw, rec, w, hh, bg)
    assert_same_bits(filled2.raw, want2)
    assert_same_bits(need2, want_need2)
    got = hd.denoise_stats(filled2, rec, w, hh)
    hd.close()
    assert_same_bits(got, SM.denoise_stats(detmath_cpu, want2, rec, w, hh, bg))
    print("classes", F.counts(F.classes(acc.raw, need, rec)), "selected", count, "then", F.counts(F.classes(acc2.raw, need2, rec)))


def test_filled_colours_beat_the_nearest_rendered_pixel(detmath_cpu):
    """wine_glass 160 x 90 (the size and converged reference of the denoiser's quality test), p8 / d16, K = 4, lattice 2: over the
    FILLED positions, which must be at least 3/4 of the EMPTY ones, the MSE of the filled colours is strictly below the MSE of
    copying the nearest rendered lattice pixel ( x - x % 2, y - y % 2 ); both of clip( x, 0, 1 ) against the converged frame.  The
    mean of matching neighbours has less noise than one of them and does not cross object edges: a relation, no margin."""
    w, hh, K, lattice = 160, 90, 4, 2
    sc = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=8, direct_samples=16)
    flat = sc.flatten()
    pos = S.positions(flat)
    n = w * hh
    hd = A.Handle(flat)
    rec = hd.surface_positions(pos, follow=True).raw
    idx = lattice_index(w, hh, lattice)
    _, part = hd.render_lens_stats(pos[idx], linear=True, samples=K, jitter=True, seed=0)
    acc = hd.lens_stats_merge(np.zeros((n, 8)), part, idx)
    filled, need = hd.fill_stats(acc, rec, w, hh)
    hd.close()
    sc.set(path_samples=4096, direct_samples=12800)
    flat = sc.flatten()
    hd = A.Handle(flat)
    ref = hd.render_positions(S.positions(flat), linear=True).reshape(hh, w, 3)
    hd.close()
    e = SM.empty(acc.raw).reshape(hh, w)
    f = F.classes(acc.raw, need, rec) == F.FILLED
    hit_empty = e & (rec[:, 0] < np.inf).reshape(hh, w)
    share = f.sum() / e.sum()
    y, x = np.mgrid[0:hh, 0:w]
    nearest = acc.raw.reshape(hh, w, 8)[y - y % lattice, x - x % lattice, 1:4]
    mse_fill = float(np.mean((np.clip(filled.raw.reshape(hh, w, 8)[f][:, 1:4], 0, 1) - np.clip(ref[f], 0, 1)) ** 2))
    mse_copy = float(np.mean((np.clip(nearest[f], 0, 1) - np.clip(ref[f], 0, 1)) ** 2))
    print(f"wine_glass {w}x{hh} K={K} lattice {lattice}: EMPTY {e.sum()} (hits {hit_empty.sum()}), FILLED {f.sum()} = {share:.3f} of the EMPTY;  "
          f"mse filled {mse_fill:.4e}  nearest rendered {mse_copy:.4e}  ({mse_fill / mse_copy:.3f})")
    assert share >= 0.75, share
    assert mse_fill < mse_copy, (mse_fill, mse_copy)


@pytest.mark.parametrize("refine", [None, 0.5])
def test_the_preview_tool(tmp_path, monkeypatch, detmath_cpu, refine):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_aovs import read_pnm
    from render_panorama import load_scene
    script = os.path.join(ROOT, "tests", "scripts", "textured.acn")
    out = tmp_path / "out.pnm"
    w, hh, K, lattice = 80, 50, 4, 2
    args = ["--lattice", str(lattice), "--samples", str(K), "--width", str(w), "--height", str(hh)] + ([] if refine is None else ["--refine-above", str(refine)])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_preview.py"), script, str(out)] + args,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    monkeypatch.chdir(tmp_path)
    flat = load_scene(script)
    prm = flat.params
    prm.image_width, prm.image_height = w, hh
    bg = np.array(prm.background_color[:])
    n = w * hh
    pos = A.main_pass_positions(w, hh)
    hd = A.Handle(flat)
    rec = hd.surface_positions(pos, follow=True).raw
    idx = lattice_index(w, hh, lattice)
    _, part = hd.render_lens_stats(pos[idx], linear=True, samples=K, jitter=True, seed=0)
    acc = hd.lens_stats_merge(np.zeros((n, 8)), part, idx)
    filled, need = hd.fill_stats(acc, rec, w, hh)
    def model_classes(acc):
        detail = {}
        F.fill(detmath_cpu, acc.raw, rec, w, hh, bg, detail=detail)
        return detail["cls"]

    models = [model_classes(acc)]
    rays = len(idx) * K
    if refine is not None:
        sel, sel_pos, count = hd.select_above(need.reshape(-1), refine, raster_width=w)
        assert count > 0
        _, part2 = hd.render_lens_stats(sel_pos, linear=True, samples=K, jitter=True, seed=1)
        acc = hd.lens_stats_merge(acc, part2, sel)
        filled, need = hd.fill_stats(acc, rec, w, hh)
        models.append(model_classes(acc))
        rays += count * K
    d = torch.from_numpy(hd.lens_stats_resolve(filled, linear=True)[0]).to("cuda")     # (an UNFILLED position shows the background)
    d_rgb8 = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    hd.resolve_dev(d.data_ptr(), n, None, d_rgb8.data_ptr())
    hd.close()
    assert not SM.empty(filled.raw).all() and np.array_equal(read_pnm(out), d_rgb8.cpu().numpy().reshape(hh, w, 3))
    # the printed counts are the model's
    printed = [dict((k, int(v)) for k, v in re.findall(r"(rendered|background|filled|unfilled) (\d+)", line))
               for line in r.stdout.splitlines() if line.startswith("fill ")]
    assert len(printed) == len(models)
    for got, cls in zip(printed, models):
        assert got == F.counts(cls), (got, F.counts(cls))
    assert f"rays: {rays} of the {n * K}" in r.stdout, r.stdout

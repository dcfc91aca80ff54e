"""Lens sample statistics without a GPU (include/actinon_hip.h: acn_render_lens_stats*, acn_lens_stats_*, acn_denoise_stats*): the
refusal of a null handle by every new entry point, the constants of the header, properties of the numpy model of
tests/stats_model.py (which test_gpu_lens_stats.py compares the device with, bit for bit), the argument parsing and the pass
selection of tools/render_progressive.py with the handle faked, and the host-side checks of actinon_amd/csrc/acn_stats_host.h in a
stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import denoise_model as D
import stats_model as T
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23
BG = np.array([0.3, 0.35, 0.4])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_entry_points_refuse_a_null_handle():
    pos, rgb, st8, surf = np.zeros((4, 2)), np.full((4, 3), 7.25), np.full((4, 8), 7.25), D.blank(4)
    part, noise = np.full((4, 8), 1.5), np.full(4, 7.25)
    idx = np.arange(4, dtype=np.int64)
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    p, dp = A.Handle.lens_params(samples=2), A.Handle.denoise_params()
    calls = {
        "acn_render_lens_stats": lambda ro: hip.acn_render_lens_stats(None, pos.ctypes.data, 4, C.byref(p), rgb.ctypes.data, st8.ctypes.data, ro),
        "acn_render_lens_stats_dev": lambda ro: hip.acn_render_lens_stats_dev(None, pos.ctypes.data, 4, C.byref(p), rgb.ctypes.data, st8.ctypes.data, ro),
        "acn_render_lens_stats_main_pass_dev": lambda ro: hip.acn_render_lens_stats_main_pass_dev(None, 0, 4, C.byref(p), rgb.ctypes.data, st8.ctypes.data, ro),
        "acn_lens_stats_merge": lambda ro: hip.acn_lens_stats_merge(None, st8.ctypes.data, 4, part.ctypes.data, 4, idx.ctypes.data, ro),
        "acn_lens_stats_merge_dev": lambda ro: hip.acn_lens_stats_merge_dev(None, st8.ctypes.data, 4, part.ctypes.data, 4, idx.ctypes.data, ro),
        "acn_lens_stats_resolve_dev": lambda ro: hip.acn_lens_stats_resolve_dev(None, st8.ctypes.data, 4, rgb.ctypes.data, noise.ctypes.data, ro),
        "acn_denoise_stats": lambda ro: hip.acn_denoise_stats(None, st8.ctypes.data, surf.ctypes.data, 2, 2, C.byref(dp), rgb.ctypes.data, ro),
        "acn_denoise_stats_dev": lambda ro: hip.acn_denoise_stats_dev(None, st8.ctypes.data, surf.ctypes.data, 2, 2, C.byref(dp), rgb.ctypes.data, ro),
    }
    assert set(calls) <= set(A._lib.HIP_SYMBOLS)
    for name, call in calls.items():
        for ro in (None, C.byref(o)):
            hip.acn_device_count()
            hip.acn_scene_upload(None, 0, None)                              # (sets another message, or none)
            assert call(ro) == abi.ACN_ERR_ARG, name
            assert b"null" in hip.acn_last_error(), (name, hip.acn_last_error())
    assert (rgb == 7.25).all() and (st8 == 7.25).all() and (noise == 7.25).all() and (part == 1.5).all()


def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    defs = dict(re.findall(r"^#define ACN_STATS_(\w+)\s+([0-9.]+)\s", text, re.M))
    assert defs == {"STRIDE": "8", "NOISE_FLOOR": "0.01"}
    assert abi.ACN_STATS_STRIDE == T.STRIDE == 8 and abi.ACN_STATS_NOISE_FLOOR == T.NOISE_FLOOR == 0.01
    assert "#define ACN_ABI_VERSION 2\n" in text and abi.ACN_ABI_VERSION == 2
    for name in ("acn_render_lens_stats_dev", "acn_render_lens_stats_main_pass_dev", "acn_render_lens_stats", "acn_lens_stats_merge_dev",
                 "acn_lens_stats_merge", "acn_lens_stats_resolve_dev", "acn_denoise_stats_dev", "acn_denoise_stats"):
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert name in A._lib.HIP_SYMBOLS and getattr(hip, name).argtypes, name
    s = A.LensStats(np.arange(16.0).reshape(2, 8))
    assert np.array_equal(s.n, [0, 8]) and np.array_equal(s.mean, [[1, 2, 3], [9, 10, 11]]) and np.array_equal(s.m2, [[4, 5, 6], [12, 13, 14]])
    assert np.isnan(s.variance_of_mean[0]).all() and np.array_equal(s.variance_of_mean[1], (np.array([12.0, 13, 14]) / 7.0) / 8.0)
    with pytest.raises(ValueError):
        A.LensStats(np.zeros((2, 7)))


# ---- properties of the model ----
def spread(rng, shape):
    """positive values over 1e-3 .. 1e3"""
    return 10.0 ** rng.uniform(-3, 3, shape)


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_equal_samples_have_no_deviation(K):
    """K equal samples: m2 == 0 exactly.  The mean is ( ( ( 0.0 + L ) + L ) + ... ) / K in the order of k, so this holds where every
    partial sum j * L is a double: always for K <= 4 (2 L and 4 L are exact, and 3 L rounds by less than half an ulp of 4 L), and
    for K = 8 for samples with three spare mantissa bits, which is what this test draws.  For arbitrary doubles at K = 8 the
    partial sums 5 L, 6 L, 7 L round, the mean can come out an ulp or two beside L, and m2 is then that step squared times K: tiny, never
    negative, and what the header defines -- the second half pins that."""
    rng = np.random.default_rng(K)
    one = spread(rng, (50, 1, 3))
    one[0] = [[0.1, 1.0 / 3.0, 1e-300]]
    any_double = one.copy()
    one = (one.view(np.uint64) & ~np.uint64(7)).view(np.float64)              # 50 significant bits
    rec = T.records(np.repeat(one, K, axis=1))
    assert (rec[:, 0] == K).all() and (rec[:, 7] == 0).all()
    assert (rec[:, 4:7] == 0.0).all() and not np.signbit(rec[:, 4:7]).any()
    assert np.array_equal(rec[:, 1:4], one[:, 0])                             # the sum and its division are exact
    rec = T.records(np.repeat(any_double, K, axis=1))
    if K <= 4:
        assert (rec[:, 4:7] == 0.0).all() and np.array_equal(rec[:, 1:4], any_double[:, 0])
    else:
        assert (rec[:, 4:7] >= 0.0).all() and (rec[:, 4:7] <= K * (2.0 ** -50 * any_double[:, 0]) ** 2).all()


def test_m2_is_never_negative_and_is_the_two_pass_sum():
    rng = np.random.default_rng(11)
    L = spread(rng, (200, 7, 3)) * rng.choice([-1.0, 1.0], (200, 7, 3))
    L[:20] = 1e3 + rng.uniform(0, 1e-9, (20, 7, 3))                           # where s2 / n - m * m cancels to nonsense
    rec = T.records(L)
    assert (rec[:, 4:7] >= 0).all()
    want = ((L - L.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    assert np.abs(rec[:, 4:7] - want).max() <= 1e-12 * np.abs(want).max()
    naive = (L * L).sum(axis=1) / 7 - L.mean(axis=1) ** 2
    assert (naive[:20] < 0).any() or np.abs(naive[:20] * 7 / want[:20] - 1).max() > 1e-3     # the form the header rules out


def test_merging_with_an_empty_record_is_the_identity():
    rng = np.random.default_rng(3)
    full = T.records(spread(rng, (6, 5, 3)))
    full[:, 7] = 0.0
    empties = np.zeros((6, 8))
    empties[1] = [0.5, 1, 2, 3, 4, 5, 6, 7]                                   # n below 1
    empties[2] = [np.nan, 1, 2, 3, 4, 5, 6, 7]
    empties[3] = [np.inf, 1, 2, 3, 4, 5, 6, 7]
    empties[4] = [-4.0, 1, 2, 3, 4, 5, 6, 7]
    empties[5, 0] = -0.0
    assert T.empty(empties).all() and not T.empty(full).any()
    assert same_bits(T.merge(full, empties), full)                            # b EMPTY: acc untouched
    assert same_bits(T.merge(empties, full), full)                            # a EMPTY: acc = b, bit for bit
    odd = full.copy()
    odd[:, 7] = 42.0                                                          # bit for bit means the reserved word too
    assert same_bits(T.merge(np.zeros((6, 8)), odd), odd)
    assert same_bits(T.merge(empties, empties), empties)
    # by index: the others keep their bits, indices out of range are skipped
    acc = T.records(spread(rng, (9, 3, 3)))
    got = T.merge(acc, full, index=[8, -1, 2, 9, 0, 4])
    rest = [1, 3, 5, 6, 7]
    assert same_bits(got[rest], acc[rest])
    assert (got[[8, 2, 0, 4], 0] == 8.0).all()


def test_split_and_merge_is_the_whole(detmath_cpu):
    rng = np.random.default_rng(7)
    K = 7
    L = spread(rng, (300, K, 3))
    whole = T.records(L)
    for k0 in range(1, K):
        got = T.merge(T.records(L[:, :k0]), T.records(L[:, k0:]))
        assert (got[:, 0] == K).all() and (got[:, 7] == 0).all()
        assert np.abs(got[:, 1:4] / whole[:, 1:4] - 1).max() <= 1e-12, k0
        assert np.abs(got[:, 4:7] / whole[:, 4:7] - 1).max() <= 1e-12, k0
    # three parts, either association
    a, b, c = T.records(L[:, :2]), T.records(L[:, 2:3]), T.records(L[:, 3:])
    left, right = T.merge(T.merge(a, b), c), T.merge(a, T.merge(b, c))
    for got in (left, right):
        assert np.abs(got[:, 1:7] / whole[:, 1:7] - 1).max() <= 1e-12
    assert np.abs(left[:, 1:7] / right[:, 1:7] - 1).max() <= 1e-12
    assert np.abs(T.noise(detmath_cpu, left) / T.noise(detmath_cpu, whole) - 1).max() <= 1e-11


def test_noise_and_resolve(detmath_cpu):
    rng = np.random.default_rng(5)
    rec = T.records(spread(rng, (8, 4, 3)))
    rec[0] = T.records(spread(rng, (1, 1, 3)))[0]                             # n = 1
    rec[1] = 0.0                                                              # EMPTY
    rec[2, 0] = np.nan
    noise = T.noise(detmath_cpu, rec)
    assert np.isposinf(noise[:3]).all() and np.isfinite(noise[3:]).all() and (noise[3:] > 0).all()
    vm = T.variance_of_mean(rec)
    assert np.isnan(vm[:3]).all() and np.array_equal(vm[3:], (rec[3:, 4:7] / 3.0) / 4.0)
    w2 = np.array([0.2126, 0.7152, 0.0722]) ** 2
    want = np.sqrt((w2 * vm[3:]).sum(axis=1)) / (np.abs(D.lum(rec[3:, 1:4])) + 0.01)
    assert np.abs(noise[3:] / want - 1).max() <= 1e-14
    lin, n2 = T.resolve(detmath_cpu, rec, BG, 0.5, True)
    assert same_bits(n2, noise) and same_bits(lin[[1, 2]], np.stack([BG, BG])) and same_bits(lin[[0, 3]], rec[[0, 3], 1:4])
    sat, _ = T.resolve(detmath_cpu, rec, BG, 0.5, False)
    assert (sat >= 0).all() and (sat <= 1).all() and np.abs(sat[1] - np.clip(BG ** 0.5, 0, 1)).max() <= 1e-15


# ---- the filter with the measured variance ----
def stats_of(lin, n=4, rel=0.1):
    """records with the frame `lin` [h,w,3] as their means: n samples, m2 as of a relative spread `rel` per sample"""
    flat = lin.reshape(-1, 3)
    rec = np.zeros((len(flat), 8))
    rec[:, 0] = n
    rec[:, 1:4] = flat
    with np.errstate(invalid="ignore"):
        m2 = (n - 1) * (rel * flat) ** 2 if n > 1 else np.zeros_like(flat)
    rec[:, 4:7] = np.where(np.isfinite(m2), m2, 0.0)
    return rec


def test_model_copies_what_it_cannot_filter(detmath_cpu):
    lin, rec = D.synthetic(W, H)
    st = stats_of(lin)
    st[5] = 0.0                                                               # an EMPTY record on a filterable pixel
    st[6, 0] = np.nan
    det = {}
    out = T.denoise_stats(detmath_cpu, st, rec, W, H, BG, detail=det)
    ok = det["ok"]
    c = (lin / D.albedo(rec).reshape(H, W, 3)).reshape(-1, 3)
    plain = D.filterable(rec, c).reshape(H, W)
    assert plain.reshape(-1)[[5, 6]].all() and not ok.reshape(-1)[[5, 6]].any()
    assert np.array_equal(ok.reshape(-1)[7:], plain.reshape(-1)[7:]) and (~plain).sum() >= 30
    keep = ~ok
    keep.reshape(-1)[[5, 6]] = False
    assert same_bits(out[keep], lin[keep])                                    # misses, emitters, the NaN and the inf pixel
    assert same_bits(out.reshape(-1, 3)[[5, 6]], np.stack([BG, BG]))          # EMPTY: the background, linear
    assert np.isfinite(out[ok]).all() and (out[ok] != lin[ok]).any(axis=-1).mean() > 0.9


def test_model_keeps_a_constant_image(detmath_cpu):
    _, rec = D.synthetic(W, H)
    value = np.array([0.3, 0.6, 0.9])
    lin = np.broadcast_to(value, (H, W, 3)).copy()
    rec = rec.copy()
    rec[:, 9:12] = [0.7, 0.2, 1.0]
    for demodulate in (True, False):
        for n in (1, 4):
            out = T.denoise_stats(detmath_cpu, stats_of(lin, n=n), rec, W, H, BG, demodulate=demodulate)
            assert np.abs(out / value - 1).max() <= 1e-15, (demodulate, n)


def one_object(h, w):
    """one flat object seen head-on: every pixel filterable, all matching"""
    rec = D.blank(h * w).reshape(h, w, 16)
    y, x = np.mgrid[0:h, 0:w]
    rec[..., 0] = 5.0
    rec[..., 1], rec[..., 2] = x * 0.1, y * 0.1
    rec[..., 6] = -1.0
    rec[..., 7] = 2
    rec[..., 9:12] = [0.5, 1.0, 0.25]
    rec[..., 12] = 2
    return rec


def test_a_single_sample_pixel_borrows_its_neighbours_variance(detmath_cpu):
    h, w = 9, 11
    rec = one_object(h, w)
    rng = np.random.default_rng(2)
    lin = 0.5 + 0.2 * rng.random((h, w, 3))
    st = stats_of(lin, n=4).reshape(h, w, 8)
    y, x = 4, 5
    st[y, x] = [1.0, *lin[y, x], 0.0, 0.0, 0.0, 0.0]
    det = {}
    T.denoise_stats(detmath_cpu, st.reshape(-1, 8), rec.reshape(-1, 16), w, h, BG, detail=det)
    vr, var = det["var_raw"], det["var"]
    assert vr[y, x] == -1.0 and (np.delete(vr.reshape(-1), y * w + x) > 0).all()
    g = np.array([0.25, 0.5, 0.25])
    wgt = np.outer(g, g)
    wgt[1, 1] = 0.0
    want = (wgt * vr[y - 1:y + 2, x - 1:x + 2]).sum() / wgt.sum()
    assert var[y, x] > 0 and abs(var[y, x] / want - 1) <= 1e-14
    # a pixel with its own measurement: the full 3 x 3 mean, weights summing to 1
    full = (np.outer(g, g) * vr[1:4, 1:4]).sum()
    assert abs(var[2, 2] / full - 1) <= 1e-14
    # the corner: four taps
    corner = (np.outer(g, g)[1:, 1:] * vr[:2, :2]).sum() / np.outer(g, g)[1:, 1:].sum()
    assert abs(var[0, 0] / corner - 1) <= 1e-14


def test_an_isolated_single_sample_pixel_is_not_smoothed_across_luminance(detmath_cpu):
    """no match in 3 x 3: var = 0, the luminance stop is at its sharpest and the pixel leaves the filter as it came in"""
    h, w = 9, 11
    rec = one_object(h, w)
    y, x = 4, 5
    rec[y, x, 7] = 3                                                          # another object: it matches nobody
    lin = np.full((h, w, 3), 0.5)
    lin[y, x] = [0.9, 0.1, 0.4]
    st = stats_of(lin, n=4).reshape(h, w, 8)
    st[y, x] = [1.0, *lin[y, x], 0.0, 0.0, 0.0, 0.0]
    det = {}
    out = T.denoise_stats(detmath_cpu, st.reshape(-1, 8), rec.reshape(-1, 16), w, h, BG, detail=det)
    assert det["ok"][y, x] and det["var"][y, x] == 0.0
    assert np.abs(out[y, x] / lin[y, x] - 1).max() <= 1e-15                   # ( c / a ) * a, roundings apart
    # and on one object, all pixels with one sample: nothing is measured anywhere, var = 0 everywhere, and a pixel that differs
    # in luminance from all its neighbours stays (exp( -|dl| / 1e-8 ) is 0)
    rec = one_object(h, w)
    st1 = stats_of(lin, n=1)
    out1 = T.denoise_stats(detmath_cpu, st1, rec.reshape(-1, 16), w, h, BG, detail=det)
    assert (det["var"] == 0).all() and (det["var_raw"] == -1.0).all()
    assert np.abs(out1[y, x] / lin[y, x] - 1).max() <= 1e-15


# ---- what it buys ----
def test_quality_against_the_oracle(oracle, detmath_cpu):
    """The gate of test_gpu_lens_stats.py on the CPU first: wine_glass_c2 at 24 x 16, the oracle's radiances of K = 4 jittered
    samples per pixel (a jittered sample without an aperture is camera_ray of the jittered position), filtered by the model with the
    model's FOLLOW records, against K = 256 jittered samples of another seed: the linear MSE over the filterable pixels is below
    that of the unfiltered mean.  Printed beside it, not asserted: acn_denoise's model on the same mean.  Seen: raw 2.79e-3,
    denoise_stats 2.28e-3, denoise 3.62e-3 (at 48 x 27: 2.09e-3, 1.19e-3, 1.76e-3)."""
    import lens_model as M
    import scenes_util as S
    import surface_model as SM
    w, h = 24, 16
    flat = A.Scene.build("wine_glass", **dict(S.SMALL["wine_glass_c2"][1], image_width=w, image_height=h)).flatten()
    pos = S.positions(flat)

    def radiances(K, seed):
        det = {}
        M.lens_rays(detmath_cpu, oracle, flat.params, pos, samples=K, jitter=True, seed=seed, detail=det)
        return oracle.render_positions(flat, det["q"].reshape(-1, 2), linear=True).reshape(len(pos), K, 3)

    st = T.records(radiances(4, 0))
    ref = M.ordered_mean(radiances(256, 9)).reshape(h, w, 3)
    rec, _ = SM.follow(oracle, flat, SM.camera_rays(flat.params, pos))
    mean = st[:, 1:4].reshape(h, w, 3)
    out = T.denoise_stats(detmath_cpu, st, rec, w, h, np.array(flat.params.background_color[:]))
    spatial = D.denoise(detmath_cpu, mean, rec)
    ok = D.filterable(rec, (mean / D.albedo(rec).reshape(h, w, 3)).reshape(-1, 3)).reshape(h, w)
    assert ok.mean() > 0.5
    mse = lambda x: float(np.mean((x[ok] - ref[ok]) ** 2))
    e_raw, e_stats, e_spatial = mse(mean), mse(out), mse(spatial)
    print(f"wine_glass_c2 {w}x{h} K=4 jitter vs K=256, oracle and models: raw {e_raw:.4e}  denoise_stats {e_stats:.4e}  denoise {e_spatial:.4e}")
    assert e_stats < e_raw, (e_stats, e_raw)


# ---- tools/render_progressive.py ----
def load_tool():
    spec = importlib.util.spec_from_file_location("render_progressive", os.path.join(ROOT, "tools", "render_progressive.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


class FakeHandle:
    """stands in for actinon_amd.Handle on CPU tensors: records the calls; a render writes records whose noise is the test's"""

    def __init__(self, noise_of_pass):
        self.calls, self.noise_of_pass, self.p = [], noise_of_pass, 0

    @staticmethod
    def view(ptr, *shape):
        return np.ctypeslib.as_array((C.c_double * int(np.prod(shape))).from_address(ptr)).reshape(shape)

    def render_lens_stats_main_pass_dev(self, first, count, d_out, d_stats, linear=False, **lens):
        self.calls.append(("main", first, count, d_out, lens))
        r = self.view(d_stats, count, 8)
        r[:] = 0.0
        r[:, 0] = lens["samples"]

    def render_lens_stats_dev(self, d_pos, n, d_out, d_stats, linear=False, **lens):
        self.calls.append(("pos", self.view(d_pos, n, 2).copy(), n, d_out, lens))
        r = self.view(d_stats, n, 8)
        r[:] = 0.0
        r[:, 0] = lens["samples"]

    def lens_stats_merge_dev(self, d_acc, n_acc, d_part, n_part, d_index):
        idx = np.ctypeslib.as_array((C.c_int64 * n_part).from_address(d_index)).copy()
        self.calls.append(("merge", idx))
        self.view(d_acc, n_acc, 8)[idx, 0] += self.view(d_part, n_part, 8)[:, 0]
        self.p += 1

    def lens_stats_resolve_dev(self, d_stats, n, d_rgb, d_noise, linear=False):
        assert d_rgb is None and linear
        self.view(d_noise, n)[:] = self.noise_of_pass[min(self.p, len(self.noise_of_pass) - 1)]


def test_progressive_tool_arguments_and_pass_selection():
    import torch
    tool = load_tool()
    a = tool.parse_args(["s.acn", "o.pnm", "--samples", "4", "--passes", "3", "--target-noise", "0.05"])
    assert (a.samples, a.passes, a.target_noise, a.denoise, a.noise_map, a.aperture) == (4, 3, 0.05, False, None, 0.0)
    a = tool.parse_args(["s.acn", "o.pnm", "--samples", "1", "--passes", "1", "--target-noise", "0", "--denoise", "--noise-map", "n.npy"])
    assert a.denoise and a.noise_map == "n.npy"
    for bad in (["--samples", "0", "--passes", "3", "--target-noise", "0.05"], ["--samples", "4097", "--passes", "3", "--target-noise", "0.05"],
                ["--samples", "4", "--passes", "0", "--target-noise", "0.05"], ["--samples", "4", "--passes", "3", "--target-noise", "-1"],
                ["--samples", "4", "--passes", "3", "--target-noise", "nan"], ["--samples", "4", "--passes", "3"],
                ["--samples", "4", "--passes", "3", "--target-noise", "0.05", "--aperture", "0.1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(["s.acn", "o.pnm"] + bad)
    assert "biased toward dark" in tool.__doc__
    # selection: strictly above the target, ascending; NaN is not above anything, +inf is above everything
    noise = torch.tensor([0.1, 0.5, 0.05, float("inf"), float("nan"), 0.2, 0.1000001], dtype=torch.float64)
    idx = tool.select(noise, 0.1)
    assert idx.dtype == torch.int64 and idx.tolist() == [1, 3, 5, 6]
    assert tool.select(noise, float("inf")).numel() == 0
    assert tool.centres(torch.tensor([0, 4, 5, 13]), 5).tolist() == [[0.5, 0.5], [4.5, 0.5], [0.5, 1.5], [3.5, 2.5]]
    # the passes: 6 x 4 pixels; after pass 0 pixels 3, 7, 20 are above the target, after pass 1 only 7, then none
    w, hh, K = 6, 4, 2
    n0 = np.zeros(24); n0[[3, 7, 20]] = 1.0
    n1 = np.zeros(24); n1[7] = 1.0
    fake = FakeHandle([n0, n1, np.zeros(24)])
    log = []
    d_acc, d_noise, rays = tool.run_passes(fake, w, hh, K, 5, 0.5, torch.device("cpu"), lens=dict(jitter=True), log=log.append)
    kinds = [c[0] for c in fake.calls]
    assert kinds == ["main", "pos", "merge", "pos", "merge"]
    assert fake.calls[0][1:3] == (0, 24) and fake.calls[0][4] == dict(samples=K, seed=0, jitter=True)
    assert np.array_equal(fake.calls[1][1], [[3.5, 0.5], [1.5, 1.5], [2.5, 3.5]]) and fake.calls[1][4]["seed"] == 1
    assert np.array_equal(fake.calls[2][1], [3, 7, 20])
    assert np.array_equal(fake.calls[3][1], [[1.5, 1.5]]) and fake.calls[3][4]["seed"] == 2 and np.array_equal(fake.calls[4][1], [7])
    assert all(c[3] is None for c in fake.calls if c[0] in ("main", "pos"))  # no colour is asked for while refining
    assert rays == [48, 6, 2] and len(log) == 4 and "no pixel" in log[-1]
    want_n = np.full(24, 2.0); want_n[[3, 20]] = 4.0; want_n[7] = 6.0
    assert np.array_equal(d_acc[:, 0].numpy(), want_n)
    # P passes at most
    fake = FakeHandle([n0])
    _, _, rays = tool.run_passes(fake, w, hh, K, 3, 0.5, torch.device("cpu"), log=log.append)
    assert rays == [48, 6, 6]
    fake = FakeHandle([n0])
    assert tool.run_passes(fake, w, hh, K, 1, 0.5, torch.device("cpu"), log=log.append)[2] == [48]


# ---- the host-side checks under the sanitizers ----
def test_host_checks_in_a_sanitized_program(tmp_path):
    """acn_stats_host.h (the index validation of acn_lens_stats_merge, the reading of acn_lens_params, the buffer checks) compiled
    with tests/csrc/stats_cpu.cpp into a program of its own with -fsanitize=address,undefined; nothing sanitized is loaded here"""
    exe = tmp_path / "stats_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "stats_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

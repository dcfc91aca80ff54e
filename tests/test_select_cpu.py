"""Selecting positions by a key, without a GPU (include/actinon_hip.h: acn_select_above*, acn_key_histogram*, acn_key_hist_edge,
acn_key_hist_threshold): the host arithmetic and the argument checks of actinon_amd/csrc/acn_select_host.h behind the shim
tests/csrc/select_cpu.cpp against the numpy model tests/select_model.py, the same file as a stand-alone program under the address and
undefined-behaviour sanitizers, the refusals of the library itself where they need no handle, and tools/render_progressive.py with
--select library and --rays-per-pass on a faked handle."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import select_model as SM
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "csrc", "select_cpu.cpp")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """acn_select_host.h compiled for the host, no sanitizer, behind the extern "C" functions of tests/csrc/select_cpu.cpp"""
    out = tmp_path_factory.mktemp("select") / "libselect_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INCLUDES + [SOURCE, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.sel_edge.argtypes, lib.sel_edge.restype = [C.c_uint32], C.c_double
    lib.sel_bins.argtypes, lib.sel_bins.restype = [C.c_void_p, C.c_size_t, C.c_void_p], None
    lib.sel_threshold.argtypes, lib.sel_threshold.restype = [C.c_void_p, C.c_uint64], C.c_double
    lib.sel_tile.restype = C.c_uint64
    lib.sel_tiles.argtypes, lib.sel_tiles.restype = [C.c_uint64], C.c_uint64
    lib.sel_check_select.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.POINTER(abi.SelectParams), C.c_char_p, C.c_size_t]
    lib.sel_check_hist.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
    return lib


def shim_bins(shim, key):
    u = bits(key).reshape(-1).copy()
    out = np.empty(len(u), dtype=np.uint32)
    shim.sel_bins(u.ctypes.data, len(u), out.ctypes.data)
    return out.astype(np.int64)


def shim_threshold(shim, hist, budget):
    hh = np.ascontiguousarray(hist, dtype=np.uint64)
    assert hh.shape == (SM.WORDS,)
    return shim.sel_threshold(hh.ctypes.data, budget)


def test_constants_mirror_the_header(shim):
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    assert dict(re.findall(r"^#define ACN_KEY_HIST_(\w+)\s+([0-9]+)\s", text, re.M)) == {"BINS": "256", "WORDS": "257"}
    assert (abi.ACN_KEY_HIST_BINS, abi.ACN_KEY_HIST_WORDS) == (SM.BINS, SM.WORDS) == (256, 257)
    assert "#define ACN_ABI_VERSION 2\n" in text and abi.ACN_ABI_VERSION == 2
    for name in ("acn_select_above_dev", "acn_select_above", "acn_key_histogram_dev", "acn_key_histogram"):
        assert re.search(r"^int " + name + r"\s*\(", text, re.M), name
        assert name in A._lib.HIP_SYMBOLS and getattr(hip, name).argtypes, name
    for name in ("acn_key_hist_edge", "acn_key_hist_threshold"):
        assert re.search(r"^double\s+" + name + r"\s*\(", text, re.M), name
        assert name in A._lib.HIP_SYMBOLS and getattr(hip, name).restype is C.c_double, name
    fields = re.search(r"typedef struct acn_select_params\s*\{(.*?)\} acn_select_params;", text, re.S).group(1)
    assert re.findall(r"^\s*(?:uint32_t|uint64_t|double)\s+(\w+);", fields, re.M) == [f[0] for f in abi.SelectParams._fields_]
    assert C.sizeof(abi.SelectParams) == 40 and abi.SelectParams.threshold.offset == 8 and abi.SelectParams.capacity.offset == 16
    tile = shim.sel_tile()
    assert 256 <= tile <= 8192 and tile & (tile - 1) == 0
    assert [shim.sel_tiles(n) for n in (0, 1, tile, tile + 1, 2 ** 31)] == [0, 1, 1, 2, 2 ** 31 // tile]


def test_edges_are_the_models_bits(shim):
    for j in list(range(0, 260)) + [2 ** 31, 2 ** 32 - 1]:
        want = SM.edge_bits(j)
        for got in (shim.sel_edge(j), hip.acn_key_hist_edge(j), A.key_hist_edge(j)):
            assert int(bits([got])[0]) == want, (j, got)
    e = np.array([SM.edge(j) for j in range(1, 256)])
    assert (np.diff(e) > 0).all() and e[0] == 2.0 ** -40
    assert np.array_equal(e[4::4] / e[:-4:4], np.full(len(e[4::4]), 2.0))     # four bins per octave
    assert np.isneginf(SM.edge(0)) and np.isnan(SM.edge(256))


def test_bins_agree_with_the_model(shim):
    e = np.array([SM.edge(j) for j in range(1, 256)])
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, -2.2250738585072014e-308,
                        np.inf, -np.inf, 1.0, -1.0, 2.0 ** -40, 1.7976931348623157e308])
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                     0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    rng = np.random.default_rng(20)
    random_bits = rng.integers(0, 2 ** 64, 100000, dtype=np.uint64).view(np.float64)
    key = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), special, nans, random_bits])
    got, want = shim_bins(shim, key), SM.key_bin(key)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    n = len(e)
    assert np.array_equal(want[:n], np.arange(1, 256)) and np.array_equal(want[n:2 * n], np.arange(0, 255))
    assert np.array_equal(want[2 * n:3 * n], np.arange(1, 256))
    s = want[3 * n:3 * n + len(special)]
    assert list(s) == [0, 0, 0, 0, 0, 0, 0, 255, 0, 161, 0, 1, 255]
    assert (want[3 * n + len(special):3 * n + len(special) + len(nans)] == 256).all()
    assert len(np.unique(want[-100000:])) > 200                                # the random patterns reach most words
    # the bin is monotone in the key, and a key is never below the edge of its bin
    srt = np.sort(random_bits[~np.isnan(random_bits)])
    b = SM.key_bin(srt)
    assert (np.diff(b) >= 0).all()
    assert (srt >= np.array([SM.edge(j) for j in range(256)])[b]).all()
    hist = SM.histogram(key)
    assert hist.dtype == np.uint64 and int(hist.sum()) == len(key) and int(hist[256]) == len(nans) + int(np.isnan(random_bits).sum())


def keys_for_thresholds(rng, n):
    key = 2.0 ** rng.uniform(-45, 6, n)
    key[rng.integers(0, n, n // 20)] = np.inf
    key[rng.integers(0, n, n // 20)] = np.nan
    key[rng.integers(0, n, n // 20)] = -key[rng.integers(0, n, n // 20)]
    key[rng.integers(0, n, n // 20)] = 0.0
    # some keys exactly on an edge: they fall out of a selection above that edge
    on = rng.integers(0, n, n // 10)
    key[on] = [SM.edge(int(j)) for j in rng.integers(1, 256, len(on))]
    return key


def test_threshold_fits_the_budget_and_is_the_lowest_that_does(shim):
    rng = np.random.default_rng(21)
    seen_inf = seen_finite = 0
    for trial in range(40):
        n = int(rng.integers(1, 3000))
        key = keys_for_thresholds(rng, n) if trial % 4 else 2.0 ** rng.uniform(-3, -1, n)   # every fourth: few bins, all crowded
        hist = SM.histogram(key)
        assert int(hist.sum()) == n
        total = n
        budgets = {0, 1, total, max(total - 1, 0), int(rng.integers(0, total + 1)), int(hist[1:256].sum()), max(int(hist[1:256].sum()) - 1, 0)}
        for budget in sorted(budgets):
            t = shim_threshold(shim, hist, budget)
            assert int(bits([t])[0]) == int(bits([SM.threshold(hist, budget)])[0]), (trial, budget)
            assert int(bits([t])[0]) == int(bits([A.key_hist_threshold(hist, budget)])[0])
            assert len(SM.select(key, t)) <= budget, (trial, budget, t)
            # it is the smallest j: the bin below would not fit
            j = 256 if np.isposinf(t) else int(SM.key_bin(np.array([t]))[0])
            assert j >= 1 and (j == 256 or SM.edge(j) == t)
            assert j == 256 or int(hist[j:256].sum()) <= budget
            if j > 1:
                assert int(hist[j - 1:256].sum()) > budget, (trial, budget, j)
            seen_inf += j == 256
            seen_finite += j < 256
    assert seen_inf > 10 and seen_finite > 10
    # words 0 and 256 never count; the ends
    hist = np.zeros(SM.WORDS, dtype=np.uint64)
    hist[0] = hist[256] = 10 ** 6
    assert shim_threshold(shim, hist, 0) == SM.edge(1) == 2.0 ** -40
    hist[255] = 3
    assert shim_threshold(shim, hist, 2) == np.inf and shim_threshold(shim, hist, 3) == SM.edge(1)
    hist[255] = hist[254] = 2 ** 64 - 1
    assert shim_threshold(shim, hist, 2 ** 64 - 1) == SM.edge(255) == SM.threshold(hist, 2 ** 64 - 1)
    assert np.isnan(hip.acn_key_hist_threshold(None, 5))
    with pytest.raises(ValueError):
        A.key_hist_threshold(np.zeros(256, dtype=np.uint64), 1)


def params(**kw):
    p = abi.SelectParams()
    p.struct_size = C.sizeof(abi.SelectParams)
    p.threshold, p.capacity = 0.5, 4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_every_refusal_names_its_reason_and_writes_nothing(shim):
    key, src, pos = np.arange(4.0), np.full((4, 2), 7.25), np.full((4, 2), 7.25)
    idx = np.full(4, 77, dtype=np.int64)
    K, S, I, P = key.ctypes.data, src.ctypes.data, idx.ctypes.data, pos.ctypes.data
    sentinel = dict(struct_size=1234, flags=99, threshold=-7.5, capacity=42, raster_width=43, raster_first=44)

    def run(word, have=1, k=K, n=4, prm=None, s=None, i=I, p=P, world=1, null_prm=False):
        out = params(**sentinel)
        msg = C.create_string_buffer(b"untouched", 256)
        q = params() if prm is None else prm
        st = shim.sel_check_select(have, k, n, None if null_prm else C.byref(q), s, i, p, world, C.byref(out), msg, 256)
        if word is None:
            assert st == abi.ACN_OK and msg.value == b"untouched", msg.value
            return out
        assert st == abi.ACN_ERR_ARG and word.encode() in msg.value, (word, st, msg.value)
        assert all(getattr(out, f) == v for f, v in sentinel.items())          # the parameters as read: written only on success
        return None

    run("handle", have=0)
    run("key", k=None)
    run("2^31", n=2 ** 31 + 1)
    run("acn_select_params", null_prm=True)
    for size in (0, 4, 8, 15):
        run("struct_size", prm=params(struct_size=size))
    run("flags", prm=params(flags=1))
    run("flags", prm=params(flags=2 ** 31))
    run("NaN", prm=params(threshold=float("nan")))
    run("capacity", i=None, p=None)
    run("sharded", world=2)
    run("align", k=K + 4)
    run("align", p=P + 2)
    run("align", s=S + 1)
    run("2^52", prm=params(raster_first=2 ** 52))
    run("2^52", prm=params(raster_first=2 ** 64 - 1))
    # what is accepted: the parameters come back as far as struct_size reaches
    got = run(None, prm=params(threshold=-np.inf, capacity=9, raster_width=5, raster_first=6))
    assert (got.threshold, got.capacity, got.raster_width, got.raster_first) == (-np.inf, 9, 5, 6)
    got = run(None, prm=params(struct_size=24, capacity=9, raster_width=5, raster_first=6))
    assert (got.threshold, got.capacity, got.raster_width, got.raster_first) == (0.5, 9, 0, 0)
    got = run(None, prm=params(struct_size=16, capacity=9), i=None, p=None)   # capacity not read: a pure count
    assert got.capacity == 0
    run(None, k=None, n=0)
    run(None, n=2 ** 31)
    run(None, prm=params(threshold=np.inf), i=None)
    run(None, prm=params(capacity=0), i=None, p=None)
    run(None, prm=params(raster_first=2 ** 52), s=S)                          # gathered positions: the raster is not used
    run(None, prm=params(raster_first=2 ** 52), p=None)

    hist = np.full(SM.WORDS, 5, dtype=np.uint64)

    def run_hist(word, have=1, k=K, n=4, out=hist.ctypes.data, world=1):
        msg = C.create_string_buffer(b"untouched", 256)
        st = shim.sel_check_hist(have, k, n, out, world, msg, 256)
        if word is None:
            assert st == abi.ACN_OK and msg.value == b"untouched"
        else:
            assert st == abi.ACN_ERR_ARG and word.encode() in msg.value, (word, msg.value)

    run_hist("handle", have=0)
    run_hist("key", k=None)
    run_hist("out_hist", out=None)
    run_hist("2^31", n=2 ** 31 + 1)
    run_hist("sharded", world=2)
    run_hist("align", k=K + 4)
    run_hist(None)
    run_hist(None, k=None, n=0)
    assert (key == np.arange(4.0)).all() and (src == 7.25).all() and (pos == 7.25).all() and (idx == 77).all() and (hist == 5).all()


def test_the_library_refuses_a_null_handle_before_anything_else():
    key, pos = np.arange(4.0), np.full((4, 2), 7.25)
    idx = np.full(4, 77, dtype=np.int64)
    hist = np.full(SM.WORDS, 5, dtype=np.uint64)
    count = C.c_uint64(123)
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    p = params()
    calls = {
        "acn_select_above_dev": lambda ro: hip.acn_select_above_dev(None, key.ctypes.data, 4, C.byref(p), None, idx.ctypes.data, pos.ctypes.data, None, C.byref(count), ro),
        "acn_select_above": lambda ro: hip.acn_select_above(None, key.ctypes.data, 4, C.byref(p), None, idx.ctypes.data, pos.ctypes.data, C.byref(count)),
        "acn_key_histogram_dev": lambda ro: hip.acn_key_histogram_dev(None, key.ctypes.data, 4, hist.ctypes.data, ro),
        "acn_key_histogram": lambda ro: hip.acn_key_histogram(None, key.ctypes.data, 4, hist.ctypes.data),
    }
    for name, call in calls.items():
        for ro in (None, C.byref(o)):
            hip.acn_scene_upload(None, 0, None)                                 # (sets another message)
            assert call(ro) == abi.ACN_ERR_ARG, name
            assert b"null" in hip.acn_last_error() and b"handle" in hip.acn_last_error(), (name, hip.acn_last_error())
    assert (pos == 7.25).all() and (idx == 77).all() and (hist == 5).all() and count.value == 123


def test_host_arithmetic_in_a_sanitized_program(tmp_path):
    """tests/csrc/select_cpu.cpp with its own main: every refusal and the ends of the histogram arithmetic, inputs in heap blocks of
    exactly their size, under -fsanitize=address,undefined -fno-sanitize-recover=all.  Nothing sanitized is loaded here."""
    exe = tmp_path / "select_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DSELECT_CPU_MAIN"] + INCLUDES + [SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- tools/render_progressive.py ----
def load_tool():
    spec = importlib.util.spec_from_file_location("render_progressive", os.path.join(ROOT, "tools", "render_progressive.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


class FakeHandle:
    """stands in for actinon_amd.Handle on CPU tensors: records the calls; a render writes records whose noise is the test's; the
    select and the histogram are the model's"""

    def __init__(self, noise_of_pass):
        self.calls, self.noise_of_pass, self.p = [], noise_of_pass, 0

    @staticmethod
    def view(ptr, *shape, ctype=C.c_double):
        return np.ctypeslib.as_array((ctype * int(np.prod(shape))).from_address(ptr)).reshape(shape)

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
        idx = self.view(d_index, n_part, ctype=C.c_int64).copy()
        self.calls.append(("merge", idx))
        self.view(d_acc, n_acc, 8)[idx, 0] += self.view(d_part, n_part, 8)[:, 0]
        self.p += 1

    def lens_stats_resolve_dev(self, d_stats, n, d_rgb, d_noise, linear=False):
        assert d_rgb is None and linear
        self.noise_ptr = d_noise
        self.view(d_noise, n)[:] = self.noise_of_pass[min(self.p, len(self.noise_of_pass) - 1)]

    def select_above_dev(self, d_key, n, threshold, capacity, d_index_ptr=None, d_pos_ptr=None, d_src_pos_ptr=None, raster_width=0,
                         raster_first=0, d_count_ptr=None, want_count=True, stream=None):
        self.calls.append(("select", dict(d_key=d_key, n=n, threshold=threshold, capacity=capacity, src=d_src_pos_ptr, width=raster_width,
                                          first=raster_first, d_count=d_count_ptr, want_count=want_count, stream=stream,
                                          has_index=d_index_ptr is not None, has_pos=d_pos_ptr is not None)))
        idx, pos, count = SM.select_above(self.view(d_key, n), threshold, capacity, width=raster_width, first=raster_first)
        if len(idx):
            self.view(d_index_ptr, len(idx), ctype=C.c_int64)[:] = idx
            self.view(d_pos_ptr, len(idx), 2)[:] = pos
        return count if want_count else None

    def key_histogram_dev(self, d_key, n, d_hist, stream=None):
        self.calls.append(("hist", d_key, n))
        self.view(d_hist, SM.WORDS, ctype=C.c_uint64)[:] = SM.histogram(self.view(d_key, n))


def test_progressive_tool_with_the_librarys_select():
    import torch
    tool = load_tool()
    base = ["s.acn", "o.pnm", "--samples", "4", "--passes", "3", "--target-noise", "0.05"]
    a = tool.parse_args(base)
    assert a.select == "torch" and a.rays_per_pass is None
    a = tool.parse_args(base + ["--select", "library", "--rays-per-pass", "1000"])
    assert a.select == "library" and a.rays_per_pass == 1000
    for bad in (["--select", "sort"], ["--rays-per-pass", "-1"], ["--rays-per-pass", "x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    # 6 x 4 pixels; after pass 0 pixels 3, 7, 20 are above the target, after pass 1 only 7, then none; a NaN and an inf on the way
    w, hh, K = 6, 4, 2
    n0 = np.zeros(24); n0[[3, 7, 20]] = [1.0, np.inf, 0.6]; n0[5] = np.nan; n0[6] = 0.5
    n1 = np.zeros(24); n1[7] = 1.0
    noises = [n0, n1, np.zeros(24)]
    runs = {}
    for mode in ("torch", "library"):
        fake, log, seen = FakeHandle(noises), [], []
        d_acc, d_noise, rays = tool.run_passes(fake, w, hh, K, 5, 0.5, torch.device("cpu"), lens=dict(jitter=True), log=log.append,
                                               select_mode=mode, on_pass=lambda p, t, idx, noise: seen.append((p, t, idx.tolist())))
        runs[mode] = (fake, d_acc.numpy().copy(), rays, log, seen)
    fake, acc, rays, log, seen = runs["library"]
    assert [c[0] for c in fake.calls] == ["main", "select", "pos", "merge", "select", "pos", "merge", "select"]
    for c in fake.calls:
        if c[0] == "select":   # the arguments of the contract: the noise on the device, every pixel, the raster of the frame
            assert c[1] == dict(d_key=fake.noise_ptr, n=24, threshold=0.5, capacity=24, src=None, width=w, first=0, d_count=None,
                                want_count=True, stream=None, has_index=True, has_pos=True)
    assert np.array_equal(fake.calls[2][1], [[3.5, 0.5], [1.5, 1.5], [2.5, 3.5]]) and np.array_equal(fake.calls[3][1], [3, 7, 20])
    assert np.array_equal(fake.calls[5][1], [[1.5, 1.5]]) and np.array_equal(fake.calls[6][1], [7])
    assert seen == [(1, 0.5, [3, 7, 20]), (2, 0.5, [7]), (3, 0.5, [])]
    t_fake, t_acc, t_rays, t_log, t_seen = runs["torch"]
    assert [c[0] for c in t_fake.calls] == ["main", "pos", "merge", "pos", "merge"]
    assert rays == t_rays == [48, 6, 2] and np.array_equal(acc, t_acc) and log == t_log and seen == t_seen
    for a, b in zip([c for c in fake.calls if c[0] != "select"], t_fake.calls):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("mode", ["torch", "library"])
def test_progressive_tool_with_a_ray_budget(mode):
    import torch
    tool = load_tool()
    w, hh, K, P = 8, 5, 2, 4
    n = w * hh
    rng = np.random.default_rng(22)
    noises = [2.0 ** rng.uniform(-8, 0, n) for _ in range(P)]
    noises[0][[4, 9]] = [np.inf, np.nan]
    target, B = 2.0 ** -6, 15                                                  # B // K = 7 positions a pass
    budget = B // K
    assert (noises[0] > target).sum() > 2 * budget                             # the budget binds
    fake, seen = FakeHandle(noises), []
    d_acc, d_noise, rays = tool.run_passes(fake, w, hh, K, P, target, torch.device("cpu"), log=lambda *_: None, select_mode=mode,
                                           rays_per_pass=B, on_pass=lambda p, t, idx, noise: seen.append((p, t, idx.tolist())))
    assert len(seen) == P - 1 and rays[0] == n * K
    hists = [c for c in fake.calls if c[0] == "hist"]
    assert len(hists) == P - 1 and all(c[1:] == (fake.noise_ptr, n) for c in hists)
    for (p, t, idx), noise, r in zip(seen, noises, rays[1:]):
        want_t = max(target, SM.threshold(SM.histogram(noise), budget))
        assert t == want_t and t > target
        assert idx == SM.select(noise, want_t).tolist() and 0 < len(idx) <= budget
        assert r == len(idx) * K <= B
    assert 4 in seen[0][2] and 9 not in seen[0][2]                             # +inf is the noisiest pixel, NaN is never taken
    selects = [c[1] for c in fake.calls if c[0] == "select"]
    assert len(selects) == (P - 1 if mode == "library" else 0)
    assert all(s["capacity"] == budget and s["n"] == n and s["width"] == w for s in selects)   # never more than B // K positions asked for
    # a budget below one position: nothing is refined
    fake = FakeHandle(noises)
    assert tool.run_passes(fake, w, hh, K, P, target, torch.device("cpu"), log=lambda *_: None, select_mode=mode, rays_per_pass=1)[2] == [n * K]

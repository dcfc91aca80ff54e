"""The device-resident frame without a GPU (include/actinon_hip.h: acn_frame_*, acn_lcg00_jump): the host arithmetic and the argument
checks of actinon_amd/csrc/acn_frame_host.h behind the shim tests/csrc/frame_cpu.cpp against the numpy model tests/frame_model.py, bit
for bit; the seeds that make a draw convert to exactly 1.0; the same file as a stand-alone program under the address and
undefined-behaviour sanitizers; the header's declarations against the binding; the refusals of the library that need no handle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import actinon_amd as A
import frame_model as FM
from actinon_amd import abi
from actinon_amd._lib import hip, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "csrc", "frame_cpu.cpp")
RASTERS = [(1, 1), (1, 5), (5, 1), (64, 4), (37, 19), (67, 41)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """acn_frame_host.h compiled for the host, no sanitizer, behind the extern "C" functions of tests/csrc/frame_cpu.cpp"""
    out = tmp_path_factory.mktemp("frame") / "libframe_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared"] + INCLUDES + [SOURCE, "-o", str(out)])
    lib = C.CDLL(str(out))
    vp, u64 = C.c_void_p, C.c_uint64
    lib.frm_jump.argtypes, lib.frm_jump.restype = [u64, u64], u64
    lib.frm_draw.argtypes, lib.frm_draw.restype = [u64], C.c_double
    lib.frm_key.argtypes, lib.frm_key.restype = [vp, u64, u64, vp], None
    lib.frm_positions.argtypes, lib.frm_positions.restype = [vp, u64, u64, u64, u64, vp], None
    lib.frm_push.argtypes, lib.frm_push.restype = [vp, u64, u64, vp, vp, u64], None
    lib.frm_target.argtypes, lib.frm_target.restype = [C.c_double, C.c_double, u64, u64], C.c_int64
    lib.frm_image.argtypes, lib.frm_image.restype = [vp, u64, vp, vp], None
    lib.frm_slice_groups.argtypes, lib.frm_slice_groups.restype = [u64, u64], u64
    for name in ("frm_max_pixels", "frm_max_samples", "frm_slice"):
        getattr(lib, name).restype = u64
    lib.frm_check_create.argtypes = [C.c_int, u64, u64, vp, C.c_char_p, C.c_size_t]
    lib.frm_check_copy.argtypes = [C.c_int, vp, C.c_char_p, C.c_size_t]
    lib.frm_check_plan.argtypes = [C.c_int, C.c_int, C.c_double, u64, C.c_char_p, C.c_size_t]
    lib.frm_check_step.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint32, u64, u64, u64, u64, C.c_int, C.c_char_p, C.c_size_t]
    lib.frm_check_pass.argtypes = [C.c_int, vp, C.c_char_p, C.c_size_t]
    lib.frm_check_view.argtypes = [C.c_int, vp, C.c_char_p, C.c_size_t]
    return lib


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 2 ** 20 + 3, 2 ** 63, 2 ** 64 - 1])
def test_jump_equals_sequential_steps(shim, n):
    """acn_lcg00_jump against n steps of x' = x * A + C: stepped one by one where that is feasible, beyond it through what n steps
    are: 2^63 steps twice and 2^64 - 1 steps plus one both come back to the seed (the generator has the full period 2^64)."""
    for seed in (0, FM.SEED, 2 ** 64 - 1, 0x0123456789ABCDEF):
        got = shim.frm_jump(seed, n)
        assert got == hip.acn_lcg00_jump(seed, n) == A.lcg00_jump(seed, n)
        if n <= 2 ** 20 + 3:
            assert got == FM.lcg_steps(seed, n), (seed, n)
        elif n == 2 ** 63:
            half = FM.lcg_steps(shim.frm_jump(seed, 2 ** 63 - 2 ** 10), 2 ** 10)     # the last 1024 of them one by one
            assert got == half and shim.frm_jump(got, 2 ** 63) == seed and got != seed
        else:
            assert FM.lcg(got) == seed


def test_constructed_seeds_reach_one(shim):
    """A draw of 2^64 - 1024 or more converts to exactly 1.0, the one below to the largest double below 1; a seed built with the
    inverse of A makes such a draw the first (or the second), and the model's push then really lands the entry in the neighbour."""
    assert (FM.A * FM.A_INV) % 2 ** 64 == 1
    for t, want in ((2 ** 64 - 1024, 1.0), (2 ** 64 - 1, 1.0), (2 ** 64 - 1025, 0.9999999999999999)):
        seed = FM.seed_for_draw(t)
        assert FM.lcg(seed) == t and shim.frm_jump(seed, 1) == t
        assert shim.frm_draw(t) == want == FM.draw_double(t), t
        assert FM.lcg(FM.lcg(FM.seed_for_draw(t, 2))) == t
    w, h, K = 4, 3, 2
    idx = np.array([5, 6], dtype=np.int64)                                      # pixels ( 1, 1 ) and ( 2, 1 )
    clr = np.arange(12.0).reshape(4, 3) / 16
    for nth, landed in ((1, 6), (2, 9)):                                        # dx == 1.0: pixel ( 2, 1 ); dy == 1.0: pixel ( 1, 2 )
        pos, _ = FM.positions(idx, K, FM.seed_for_draw(2 ** 64 - 1, nth), w)
        assert pos[0][0 if nth == 1 else 1] == 2.0                              # pixel 1 + exactly 1.0
        acc, target = FM.push(np.zeros((w * h, 6)), w, h, pos, clr)
        assert target[0] == landed and target[1] == 5 and list(target[2:]) == [6, 6]
        assert acc[landed, 5] == (3.0 if landed == 6 else 1.0) and acc[5, 5] == 1.0
        assert shim.frm_target(pos[0][0], pos[0][1], w, h) == landed
    # the largest draw below 1.0 stays in column 0; from column 1 on the SUM i + dx rounds up to the neighbour as well (a tie to even)
    pos, _ = FM.positions(np.array([4, 6], dtype=np.int64), K, FM.seed_for_draw(2 ** 64 - 1025), w)
    assert pos[0][0] == 0.9999999999999999 and FM.push(np.zeros((w * h, 6)), w, h, pos, clr)[1][0] == 4
    pos, _ = FM.positions(idx, K, FM.seed_for_draw(2 ** 64 - 1025), w)
    assert pos[0][0] == 2.0 and FM.push(np.zeros((w * h, 6)), w, h, pos, clr)[1][0] == 6


@pytest.mark.parametrize("w,h", RASTERS)
def test_host_steps_are_the_models_bits(shim, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    n = w * h
    acc = FM.random_frame(rng, w, h)
    if n >= 5:
        acc[rng.integers(0, n)] = 0.0                                           # a record with weight 0 for certain
    key = np.empty(n)
    shim.frm_key(acc.ctypes.data, w, h, key.ctypes.data)
    want_key = FM.key(acc, w, h)
    assert same_bits(key, want_key)
    if n == 1 or w == 1 and h == 1:
        assert key[0] == 0.0
    thresholds = [np.inf, -np.inf, float(np.median(want_key))]
    for K in (1, 2, 3):
        for thr in thresholds:
            idx = FM.select(want_key, thr)
            assert len(idx) == (0 if thr == np.inf else n if thr == -np.inf else len(idx))
            rval = FM.SEED + K
            want_pos, want_rval = FM.positions(idx, K, rval, w)
            pos = np.empty((len(idx) * K, 2))
            shim.frm_positions(idx.ctypes.data, len(idx), K, rval, w, pos.ctypes.data)
            assert same_bits(pos, want_pos)
            assert shim.frm_jump(rval, 2 * K * len(idx)) == want_rval
            clr = rng.uniform(0, 2, (len(pos), 3))
            got = acc.copy()
            shim.frm_push(got.ctypes.data, w, h, pos.ctypes.data, clr.ctypes.data, len(pos))
            want, _ = FM.push(acc, w, h, pos, clr)
            assert same_bits(got, want)
            rgb, rgb8 = np.empty((n, 3)), np.empty((n, 3), dtype=np.uint8)
            shim.frm_image(got.ctypes.data, n, rgb.ctypes.data, rgb8.ctypes.data)
            want_rgb, want_rgb8 = FM.image(want)
            assert same_bits(rgb, want_rgb) and np.array_equal(rgb8, want_rgb8)
            assert np.array_equal(rgb8, A.cps_from_cl(want_rgb))
            for p in range(0, n, max(1, n // 7)):                               # the driver's own acn_cps_from_cl, pixel by pixel
                v = host.acn_cps_from_cl(want_rgb[p].ctypes.data_as(C.POINTER(C.c_double)))
                assert [v & 255, (v >> 8) & 255, (v >> 16) & 255] == list(rgb8[p])


def test_image_of_special_values(shim):
    acc = np.zeros((6, 6))
    acc[:, 5] = [0.0, 2.0, 1.0, 1.0, 4.0, 1.0]
    acc[:, 2] = [0.7, 1.0, np.nan, -0.5, 8.0, 1.0 / 256]
    acc[:, 3] = [3.0, 1.999, np.inf, 0.0, 3.999, 0.999999]
    rgb, rgb8 = np.empty((6, 3)), np.empty((6, 3), dtype=np.uint8)
    shim.frm_image(acc.ctypes.data, 6, rgb.ctypes.data, rgb8.ctypes.data)
    want_rgb, want_rgb8 = FM.image(acc)
    assert same_bits(rgb, want_rgb) and np.array_equal(rgb8, want_rgb8)
    assert rgb8[:, 0].tolist() == [179, 128, 0, 0, 255, 1] and rgb8[:, 1].tolist() == [255, 255, 255, 0, 255, 255]


def test_every_refusal_names_its_reason(shim):
    buf = C.create_string_buffer(64)
    ptr = C.addressof(buf)

    def run(fn, word, *args):
        msg = C.create_string_buffer(b"untouched", 256)
        st = fn(*args, msg, 256)
        if word is None:
            assert st == abi.ACN_OK and msg.value == b"untouched", msg.value
        else:
            assert st == abi.ACN_ERR_ARG and word.encode() in msg.value, (word, st, msg.value)

    big = shim.frm_max_pixels()
    assert big == 2 ** 31 and shim.frm_max_samples() == 2 ** 16 and shim.frm_slice() == 2 ** 24
    run(shim.frm_check_create, "handle", 0, 4, 4, ptr)
    run(shim.frm_check_create, "out", 1, 4, 4, None)
    run(shim.frm_check_create, "width", 1, 0, 4, ptr)
    run(shim.frm_check_create, "height", 1, 4, 0, ptr)
    run(shim.frm_check_create, "2^31", 1, big, 1, ptr)
    run(shim.frm_check_create, "2^31", 1, 1, big, ptr)
    run(shim.frm_check_create, "2^31", 1, 2 ** 16, 2 ** 15 + 1, ptr)
    run(shim.frm_check_create, "2^31", 1, 2 ** 33, 2 ** 33, ptr)                # a product that wraps
    run(shim.frm_check_create, None, 1, 2 ** 16, 2 ** 15, ptr)
    run(shim.frm_check_create, None, 1, 1, 1, ptr)
    run(shim.frm_check_copy, "frame", 0, ptr)
    run(shim.frm_check_copy, "lum", 1, None)
    run(shim.frm_check_copy, None, 1, ptr)
    run(shim.frm_check_plan, "frame", 0, 0, 0.1, 1)
    run(shim.frm_check_plan, "samples is 0", 1, 0, 0.1, 0)
    run(shim.frm_check_plan, "65536", 1, 0, 0.1, 2 ** 16 + 1)
    run(shim.frm_check_plan, "NaN", 1, 0, float("nan"), 1)
    run(shim.frm_check_plan, "consumed", 1, 1, 0.1, 1)
    run(shim.frm_check_plan, None, 1, 0, -np.inf, 2 ** 16)
    run(shim.frm_check_plan, None, 1, 0, np.inf, 1)
    run(shim.frm_check_step, "frame", 0, 1, b"push", 0, 0, 0, 0, 0, 0)
    run(shim.frm_check_step, "push without a plan", 1, 0, b"push", 0, 0, 0, 0, 0, 0)
    run(shim.frm_check_step, "render without a plan", 1, 0, b"render", 0, 4, 4, 4, 4, 1)
    run(shim.frm_check_step, "sharded", 1, 1, b"render", 2, 4, 4, 4, 4, 1)
    run(shim.frm_check_step, "the frame is 4 x 4, the raster of the resident scene 8 x 4", 1, 1, b"render", 1, 4, 4, 8, 4, 1)
    run(shim.frm_check_step, None, 1, 1, b"render", 1, 4, 4, 4, 4, 1)
    run(shim.frm_check_step, None, 1, 1, b"push", 0, 4, 4, 8, 8, 0)
    run(shim.frm_check_pass, "frame", 0, ptr)
    run(shim.frm_check_pass, "rval", 1, None)
    run(shim.frm_check_pass, None, 1, ptr)
    small = C.c_uint32(4)
    run(shim.frm_check_view, "struct_size", 1, C.addressof(small))
    run(shim.frm_check_view, "out", 1, None)
    b = abi.FrameBuffers()
    b.struct_size = C.sizeof(b)
    run(shim.frm_check_view, "frame", 0, C.addressof(b))
    run(shim.frm_check_view, None, 1, C.addressof(b))
    assert [shim.frm_slice_groups(s, k) for s, k in ((10, 3), (2, 3), (2 ** 24, 1), (2 ** 24, 2 ** 16))] == [3, 1, 2 ** 24, 256]


def test_the_library_refuses_nulls_before_anything_else():
    out, rv, fl = C.c_void_p(123), C.c_uint64(7), C.c_uint64(9)
    lum = np.full(12, 2.5)
    o = abi.RenderOpts()
    o.struct_size = C.sizeof(abi.RenderOpts)
    b = abi.FrameBuffers()
    b.struct_size = C.sizeof(b)
    calls = {
        "acn_frame_create": (lambda: hip.acn_frame_create(None, 4, 4, C.byref(out)), b"handle"),
        "acn_frame_upload": (lambda: hip.acn_frame_upload(None, lum.ctypes.data), b"frame"),
        "acn_frame_download": (lambda: hip.acn_frame_download(None, lum.ctypes.data), b"frame"),
        "acn_frame_main_pass": (lambda: hip.acn_frame_main_pass(None, C.byref(o)), b"frame"),
        "acn_frame_plan": (lambda: hip.acn_frame_plan(None, 0.1, 1, 5, C.byref(fl), C.byref(rv)), b"frame"),
        "acn_frame_render": (lambda: hip.acn_frame_render(None, C.byref(o)), b"frame"),
        "acn_frame_push": (lambda: hip.acn_frame_push(None), b"frame"),
        "acn_frame_pass": (lambda: hip.acn_frame_pass(None, 0.1, 1, C.byref(rv), C.byref(fl), C.byref(o)), b"frame"),
        "acn_frame_image": (lambda: hip.acn_frame_image(None, lum.ctypes.data, None), b"frame"),
        "acn_frame_view": (lambda: hip.acn_frame_view(None, C.byref(b)), b"frame"),
    }
    for name, (call, word) in calls.items():
        hip.acn_scene_upload(None, 0, None)                                     # (sets another message)
        assert call() == abi.ACN_ERR_ARG, name
        assert b"null" in hip.acn_last_error() and word in hip.acn_last_error(), (name, hip.acn_last_error())
    hip.acn_frame_free(None)                                                    # a no-op
    assert out.value == 123 and rv.value == 7 and fl.value == 9 and (lum == 2.5).all()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "actinon_hip.h")).read()
    assert "#define ACN_ABI_VERSION 2\n" in text and abi.ACN_ABI_VERSION == 2
    names = ["acn_frame_create", "acn_frame_upload", "acn_frame_download", "acn_frame_main_pass", "acn_frame_plan", "acn_frame_render",
             "acn_frame_push", "acn_frame_pass", "acn_frame_image", "acn_frame_view"]
    for name in names:
        m = re.search(r"^int\s+" + name + r"\s*\((.*?)\);", text, re.M | re.S)
        assert m, name
        assert name in A._lib.HIP_SYMBOLS and len(getattr(hip, name).argtypes) == len(m.group(1).split(",")), name
    assert re.search(r"^void acn_frame_free\( acn_frame\* f \);", text, re.M) and hip.acn_frame_free.restype is None
    assert re.search(r"^uint64_t acn_lcg00_jump\( uint64_t rval, uint64_t draws \);", text, re.M)
    assert hip.acn_lcg00_jump.restype is C.c_uint64 and "acn_lcg00_jump" in A._lib.HIP_SYMBOLS and "acn_frame_free" in A._lib.HIP_SYMBOLS
    fields = re.search(r"typedef struct acn_frame_buffers\s*\{(.*?)\} acn_frame_buffers;", text, re.S).group(1)
    declared = []
    for kind, members in re.findall(r"^\s*(uint32_t|uint64_t|void\*)\s+([\w, ]+);", fields, re.M):
        declared += [(m.strip(), kind) for m in members.split(",")]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "void*": C.c_void_p}
    assert [(n, ctype[k]) for n, k in declared] == list(abi.FrameBuffers._fields_)
    assert C.sizeof(abi.FrameBuffers) == 80
    scene_h = open(os.path.join(ROOT, "include", "acn_scene.h")).read()
    assert "extern int acn_scene_s_host_cycles_g;" in scene_h and re.search(r"^int acn_write_pnm8\(", scene_h, re.M)
    assert "acn_write_pnm8" in A._lib.HOST_SYMBOLS
    g = C.c_int.in_dll(host, "acn_scene_s_host_cycles_g")
    was = A.set_host_cycles(True)
    assert g.value == 1 and A.set_host_cycles(was) is True and g.value == (1 if was else 0)
    for name in ("Frame", "lcg00_jump", "set_host_cycles"):
        assert name in A.__all__


def test_pnm8_writes_the_bytes_of_the_float_writer(tmp_path):
    rng = np.random.default_rng(5)
    w, h = 7, 5
    rgb = rng.uniform(-0.2, 1.2, (w * h, 3))
    rgb8 = A.cps_from_cl(rgb)
    a, b = tmp_path / "a.pnm", tmp_path / "b.pnm"
    assert host.acn_write_pnm(str(a).encode(), rgb.ctypes.data, w, h) == abi.ACN_OK
    assert host.acn_write_pnm8(str(b).encode(), rgb8.ctypes.data, w, h) == abi.ACN_OK
    assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) == len(b"P6\n7 5\n255\n") + w * h * 3
    assert host.acn_write_pnm8(str(tmp_path / "no" / "dir.pnm").encode(), rgb8.ctypes.data, w, h) == abi.ACN_ERR_ARG


def test_host_arithmetic_in_a_sanitized_program(tmp_path):
    """tests/csrc/frame_cpu.cpp with its own main under -fsanitize=address,undefined -fno-sanitize-recover=all: every step on heap
    blocks of exactly their size, the refusals, the draws at the top of the range.  Nothing sanitized is loaded here."""
    exe = tmp_path / "frame_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DFRAME_CPU_MAIN"] + INCLUDES + [SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

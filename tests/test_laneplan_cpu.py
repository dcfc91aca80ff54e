"""The lane plan of a handle (acn_lane_plan, actinon_amd/csrc/acn_queueplan.h) without a GPU, behind the shim
tests/csrc/laneplan_cpu.cpp: how many concurrent lanes a large call gets and the persistent grids of a lane, from ACN_LANES (set or
not), the compute units of the device and the three grid overrides.  Compared value for value with a Python model; ACN_LANES=6 is the
arrangement of the rounds before the default changed; the shapes of the GPU tests that say they run on lanes keep their lane counts
under the new default; and the same file with its own main runs under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "csrc", "laneplan_cpu.cpp")
U32 = 1 << 32


@pytest.fixture(scope="module")
def lp(tmp_path_factory):
    out = tmp_path_factory.mktemp("laneplan") / "liblaneplan_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared"] + INCLUDES + [SOURCE, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.lp_lane_plan.restype, lib.lp_lane_plan.argtypes = None, [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
    for name in ("lp_default_lanes", "lp_default_lane_wgs", "lp_max_lanes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, []
    lib.lp_lanes_for_counts.restype, lib.lp_lanes_for_counts.argtypes = C.c_int, [C.c_int, C.c_uint64, C.c_uint64]
    return lib


def plan(lp, lanes, cus, grid=0, shade_grid=0, walk_grid=0):
    """lanes: None = ACN_LANES is not set"""
    out = (C.c_uint32 * 4)()
    lp.lp_lane_plan(0 if lanes is None else 1, 0 if lanes is None else lanes, cus, grid, shade_grid, walk_grid, out)
    return tuple(out)


def m_plan(default_lanes, default_wgs, max_lanes, lanes, cus, grid=0, shade_grid=0, walk_grid=0):
    """The rule in words: without ACN_LANES the default count on default_wgs workgroups per compute unit, k_shade too; with it the
    host's count (1 .. max_lanes) on one workgroup per compute unit, k_shade one and a half; a grid that is given is taken as it is,
    and k_walk follows the lanes' grid unless it has its own."""
    if lanes is None:
        n, g, s = default_lanes, cus * default_wgs % U32, cus * default_wgs % U32
    else:
        n, g, s = min(max(lanes, 1), max_lanes), cus, (cus * 3 % U32) // 2
    g = grid or g
    return n, g, shade_grid or s, walk_grid or g


def test_lane_plan_equals_its_model(lp):
    dl, dw, ml = lp.lp_default_lanes(), lp.lp_default_lane_wgs(), lp.lp_max_lanes()
    assert 1 <= dl <= 4 and dw >= 1 and ml == 16   # a default that fits HIP's four hardware queues beside the caller's stream
    for lanes in [None] + list(range(1, 17)):
        for cus in range(1, 305):
            for over in range(8):
                g, s, w = (777 if over & 1 else 0), (555 if over & 2 else 0), (333 if over & 4 else 0)
                assert plan(lp, lanes, cus, g, s, w) == m_plan(dl, dw, ml, lanes, cus, g, s, w), (lanes, cus, over)
    # a count outside 1 .. 16 is clamped, as the tunable was
    for lanes, want in ((0, 1), (-5, 1), (17, 16), (1000, 16)):
        assert plan(lp, lanes, 256)[0] == want


def test_six_given_lanes_are_the_former_arrangement(lp):
    for cus in (1, 3, 64, 255, 256, 304):
        assert plan(lp, 6, cus) == (6, cus, cus * 3 // 2, cus)
    # ... and every given count runs on those grids: a test that sets ACN_LANES renders on the grids it always had
    for lanes in range(1, 17):
        assert plan(lp, lanes, 256)[1:] == (256, 384, 256)


def test_default_plan_does_not_depend_on_an_unset_value(lp):
    dl, dw = lp.lp_default_lanes(), lp.lp_default_lane_wgs()
    out = (C.c_uint32 * 4)()
    for junk in (-1, 0, 6, 99):
        lp.lp_lane_plan(0, junk, 256, 0, 0, 0, out)
        assert tuple(out) == (dl, 256 * dw, 256 * dw, 256 * dw)


def test_gpu_tests_that_say_lanes_get_lanes_under_the_default(lp):
    """tests/test_queueplan_cpu.py::test_gpu_tests_that_say_lanes_get_lanes with the new default in the place of the six lanes of a
    test that sets no ACN_LANES.  Those that name a count keep it (a given count is the host's); of those that name none, only
    test_render_lens_is_the_ordered_mean_of_its_rays needs more than one lane, and says two."""
    lanes = lp.lp_lanes_for_counts
    dl = plan(lp, None, 256)[0]
    n = 320 * 180
    for given in (1, 2, 3, 4, 6):
        assert plan(lp, given, 256)[0] == given
    assert lanes(4, n, 64) == 3 and lanes(3, n, 64) == 3 and lanes(1, n, 64) == 1
    assert lanes(3, 4096, 64) == 1
    assert lanes(2, n, 64) == 2 and lanes(4, 256 * 256, 256) == 4
    # the shapes rendered without ACN_LANES: the counts they had under six lanes, with the default
    assert lanes(dl, n, 64) == min(dl, 3) and lanes(dl, 20000, 64) == 1
    assert lanes(dl, 96 * 54 * 8, 64) == 2 and lanes(1, 96 * 54 * 8, 64) == 1
    assert lanes(dl, 700 * 4, 64) == 1 and lanes(dl, 130 * 33, 64) == 1


def test_lane_plan_in_a_sanitized_program(tmp_path):
    """tests/csrc/laneplan_cpu.cpp with its own main under -fsanitize=address,undefined -fno-sanitize-recover=all.  Nothing sanitized
    is loaded here."""
    exe = tmp_path / "laneplan_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DLANEPLAN_CPU_MAIN"] + INCLUDES + [SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

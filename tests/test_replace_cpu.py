"""The host-only rules of a change of scene on a live handle (acn_scene_replace, acn_scene_set_params) without a GPU, behind the shim
tests/csrc/replace_cpu.cpp: the rule that decides whether the runners keep what they learned (acn_replace_keeps_learned,
actinon_amd/csrc/acn_queueplan.h) against a Python model, and the two functions acn_scene_set_params takes from the tables unit
(acn_tables_validate_params, acn_tables_levels) against what the whole-scene path says about a scene with the same parameters.  The
same file with its own main runs under the address and undefined-behaviour sanitizers.  And the new entry points refuse a null
handle before they touch a device."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import actinon_amd as A
from actinon_amd import abi
from actinon_amd._lib import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCES = [os.path.join(ROOT, "tests", "csrc", "replace_cpu.cpp"), os.path.join(ROOT, "actinon_amd", "csrc", "acn_tables.cpp")]
MEMBERS = ["n_nodes", "n_elems", "n_lights", "n_levels", "prune", "path_samples", "direct_samples", "trace_depth", "trace_min_intensity"]
MAX_DEPTH = 60                                    # 10 * ACN_MAX_PATH_LEVELS + 10 (actinon_amd/csrc/acn_counts.h)


class Kind(C.Structure):                          # acn_scene_kind
    _fields_ = [("n_nodes", C.c_uint32), ("n_elems", C.c_uint32), ("n_lights", C.c_uint64), ("n_levels", C.c_int32), ("prune", C.c_int32),
                ("path_samples", C.c_uint64), ("direct_samples", C.c_uint64), ("trace_depth", C.c_uint64), ("trace_min_intensity", C.c_double)]


@pytest.fixture(scope="module")
def rc(tmp_path_factory):
    out = tmp_path_factory.mktemp("replace") / "libreplace_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared"] + INCLUDES + SOURCES + ["-o", str(out)])
    lib = C.CDLL(str(out))
    lib.rc_kind_size.restype = C.c_size_t
    lib.rc_keeps_learned.argtypes = [C.POINTER(Kind), C.POINTER(Kind)]
    lib.rc_validate_params.argtypes = [C.POINTER(abi.Params)]
    lib.rc_levels.argtypes = [C.POINTER(abi.Params)]
    lib.rc_scene_status.argtypes = [C.POINTER(abi.Params), C.POINTER(C.c_int)]
    return lib


def bits(x):
    return struct.pack("d", x)


def m_keeps(a, b):
    """every member equal, the double by its bit pattern"""
    return int(all(bits(a[m]) == bits(b[m]) if m == "trace_min_intensity" else a[m] == b[m] for m in MEMBERS))


def next_double(x):
    return struct.unpack("d", struct.pack("Q", struct.unpack("Q", struct.pack("d", x))[0] + 1))[0]


BASE = dict(n_nodes=18, n_elems=12, n_lights=2, n_levels=2, prune=1, path_samples=64, direct_samples=50, trace_depth=11, trace_min_intensity=0.01)
CHANGES = [dict(), dict(n_nodes=19), dict(n_elems=13), dict(n_lights=3), dict(n_levels=1), dict(prune=0), dict(path_samples=16),
           dict(direct_samples=51), dict(trace_depth=21), dict(trace_min_intensity=next_double(0.01)), dict(trace_min_intensity=0.0),
           dict(trace_min_intensity=-0.0), dict(n_lights=2 + (1 << 32)), dict(path_samples=64 + (1 << 32)), dict(n_nodes=19, n_elems=13)]


def test_kind_rule_against_the_model(rc):
    """Each member changed alone, trace_min_intensity differing in its last bit, -0.0 against 0.0, a difference in the upper half of a
    64-bit member; every pair of the table, both ways."""
    assert rc.rc_kind_size() == C.sizeof(Kind)
    table = [dict(BASE, **c) for c in CHANGES]
    kept = 0
    for a in table:
        for b in table:
            want = m_keeps(a, b)
            assert rc.rc_keeps_learned(C.byref(Kind(**a)), C.byref(Kind(**b))) == want, (a, b)
            kept += want
    assert kept == len(table)                     # a kind is kept against itself alone: every entry of the table differs from every other
    zero, minus = dict(BASE, trace_min_intensity=0.0), dict(BASE, trace_min_intensity=-0.0)
    assert 0.0 == -0.0 and rc.rc_keeps_learned(C.byref(Kind(**zero)), C.byref(Kind(**minus))) == 0


def params(**kw):
    p = abi.Params()
    C.memmove(C.addressof(p), C.addressof(A.Scene.build("primitives").prm), C.sizeof(abi.Params))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_param_checks_and_levels_against_the_whole_scene_path(rc):
    """acn_tables_validate_params gives the status acn_tables_validate gives a valid scene with those parameters, and acn_tables_levels
    the levels acn_tables_build plans for it; the values themselves against the rule of the reference (a level per ten of depth
    beyond the first ten, one level without path samples)."""
    cases = [dict(trace_depth=d, path_samples=s) for d in (0, 1, 9, 10, 11, 20, 21, 30, 31, 59, MAX_DEPTH, MAX_DEPTH + 1, 1000) for s in (0, 1, 64)]
    cases += [dict(experimental_level=1), dict(experimental_level=-1), dict(image_height=1), dict(image_height=0), dict(image_width=0),
              dict(image_height=2, image_width=1), dict(image_height=1, experimental_level=1), dict(image_height=1, trace_depth=1000)]
    for kw in cases:
        p = params(**kw)
        levels = C.c_int(-1)
        st = rc.rc_scene_status(C.byref(p), C.byref(levels))
        assert rc.rc_validate_params(C.byref(p)) == st, kw
        if p.experimental_level != 0:
            want = abi.ACN_ERR_UNSUPPORTED
        elif p.image_height < 2 or p.image_width < 1:
            want = abi.ACN_ERR_ARG
        else:
            want = abi.ACN_ERR_UNSUPPORTED if p.trace_depth > MAX_DEPTH else abi.ACN_OK
        assert st == want, kw
        if st == abi.ACN_OK:
            d = p.trace_depth
            assert rc.rc_levels(C.byref(p)) == levels.value == (1 + (d - 10 + 9) // 10 if p.path_samples and d > 10 else 1), kw


def test_rules_in_a_sanitized_program(tmp_path):
    """tests/csrc/replace_cpu.cpp with its own main under -fsanitize=address,undefined -fno-sanitize-recover=all, the tables unit
    compiled with it.  Nothing sanitized is loaded here."""
    exe = tmp_path / "replace_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DREPLACE_CPU_MAIN"] + INCLUDES + SOURCES + ["-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_new_entry_points_refuse_null_before_any_device():
    """acn_scene_replace, acn_scene_set_params and acn_scene_info with a null handle (and with null everything) are ACN_ERR_ARG:
    the check comes before the device is touched, so this holds with and without a GPU."""
    flat = A.Scene.build("primitives").flatten()
    out = (C.c_uint64 * abi.ACN_INFO_N)()
    assert hip.acn_scene_replace(None, C.byref(flat.c), 0) == abi.ACN_ERR_ARG
    assert hip.acn_scene_replace(None, None, abi.ACN_REPLACE_FORGET) == abi.ACN_ERR_ARG
    assert hip.acn_scene_set_params(None, C.byref(flat.c.params)) == abi.ACN_ERR_ARG
    assert hip.acn_scene_set_params(None, None) == abi.ACN_ERR_ARG
    assert hip.acn_scene_info(None, out, abi.ACN_INFO_N) == abi.ACN_ERR_ARG
    assert b"null" in hip.acn_last_error() or b"bad argument" in hip.acn_last_error()
    assert len(A.Handle.INFO) == abi.ACN_INFO_N

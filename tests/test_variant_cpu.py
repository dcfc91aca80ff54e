"""The variant dispatch of the launch wrappers (actinon_amd/csrc/acn_variant.h) without a GPU, behind the shim tests/csrc/variant_cpu.cpp.
The variants of a kernel compute the same bits, so no GPU test can tell a wrapper that launches < L, P > from one that launches
< P, L >; what can be checked is the dispatch: for every combination of flags the callable runs exactly once and receives, as
compile-time constants, exactly the values passed, each at the position it was passed in.  The shim answers
calls * 1000 + first * 100 + second * 10 + third with a position's digit 1 for false, 2 for true and 0 where the form has none.  The same
file with its own main runs under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "actinon_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "csrc", "variant_cpu.cpp")


@pytest.fixture(scope="module")
def vc(tmp_path_factory):
    out = tmp_path_factory.mktemp("variant") / "libvariant_cpu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared"] + INCLUDES + [SOURCE, "-o", str(out)])
    lib = C.CDLL(str(out))
    for name, n in (("vc_one", 1), ("vc_pair", 2), ("vc_triple", 3)):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, [C.c_int] * n
    return lib


def expected(flags):
    digits = [2 if f else 1 for f in flags] + [0] * (3 - len(flags))
    return 1000 + digits[0] * 100 + digits[1] * 10 + digits[2]


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=3)))
def test_triple_is_called_once_with_the_constants_in_order(vc, flags):
    assert vc.vc_triple(*map(int, flags)) == expected(flags)


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=2)))
def test_pair_is_called_once_with_the_constants_in_order(vc, flags):
    assert vc.vc_pair(*map(int, flags)) == expected(flags)


@pytest.mark.parametrize("flag", (False, True))
def test_single_flag_is_called_once_with_its_constant(vc, flag):
    assert vc.vc_one(int(flag)) == expected((flag,))


def test_any_nonzero_int_of_the_shim_is_true(vc):
    """(the shim's own conversion, so that the cases above mean what they say)"""
    assert vc.vc_triple(7, 0, -1) == expected((True, False, True))


def test_dispatch_in_a_sanitized_program(tmp_path):
    """tests/csrc/variant_cpu.cpp with its own main under -fsanitize=address,undefined -fno-sanitize-recover=all: all eight triples, four
    pairs and both single flags.  Nothing sanitized is loaded here."""
    exe = tmp_path / "variant_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DVARIANT_CPU_MAIN"] + INCLUDES + [SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

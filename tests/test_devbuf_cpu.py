"""The owning types of the handle's device memory, events and streams (actinon_amd/csrc/acn_devbuf.h) without a GPU:
tests/csrc/devbuf_cpu.cpp puts them on a counting allocator over malloc and runs as a stand-alone program under the address and
undefined-behaviour sanitizers, whose leak check sees whatever the types lose.  Nothing sanitized is loaded here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "csrc", "devbuf_cpu.cpp")
HEADER = os.path.join(ROOT, "actinon_amd", "csrc", "acn_devbuf.h")


def test_owners_free_once_and_lose_nothing_in_a_sanitized_program(tmp_path):
    """grow within the capacity, a larger grow (freed, then allocated), a failed allocation, moves, the allocate / release whole /
    halve / allocate round of ensure_workspace with allocation 7 failing, and the owners of an event and a stream"""
    exe = tmp_path / "devbuf_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "actinon_amd", "csrc"), SOURCE, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_the_header_is_host_only():
    """no HIP header and no HIP call: allocation and release come through the policy alone"""
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipMalloc" not in text and "hipFree" not in text

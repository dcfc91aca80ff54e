"""The CPU side of the hard-ray stage tests (tests/test_gpu_stages_hard.py): the planning and the argument checks of ACN_STAGE_HARD_SHADOW
and ACN_STAGE_HARD_PATH in a sanitized program, and the queue layouts the GPU test hands to the kernels, from what the kernels' fill
phase does with them (tests/hard_queues.py: a model of the pending list)."""
import os
import subprocess

import numpy as np

import actinon_amd as A
import hard_queues as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hard_stage_checks_in_a_sanitized_program(tmp_path):
    """acn_stage_host.h compiled with tests/csrc/stage_hard_cpu.cpp into a program of its own with -fsanitize=address,undefined: every
    refusal of the two hard-ray stages and the plan of an accepted call, records in heap blocks of exactly their size; nothing
    sanitized is loaded here"""
    exe = tmp_path / "stage_hard_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "actinon_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "stage_hard_cpu.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_binding_names_the_new_stages_and_word():
    assert (A.abi.ACN_STAGE_SHADE_HITS, A.abi.ACN_STAGE_SHADE, A.abi.ACN_STAGE_HARD_SHADOW, A.abi.ACN_STAGE_HARD_PATH) == (0, 1, 2, 3)
    with open(os.path.join(ROOT, "include", "actinon_hip.h")) as f:
        assert "ACN_STAGE_HARD_SHADOW = 2, ACN_STAGE_HARD_PATH = 3, ACN_STAGE_N" in f.read()
    with open(os.path.join(ROOT, "actinon_amd", "csrc", "acn_counts.h")) as f:
        assert f"QS_DEAD_HS = {A.abi.QS_DEAD_HS}," in f.read()
    assert A.abi.QS_DEAD_HS not in A.Handle.QC.values()        # a free word of the block


def test_layouts_reach_the_list_states_they_are_named_for():
    """Every layout of the GPU test, run through the model of a wave's two phases: the list never holds more than 127 indices, and
    each layout produces the state it is there for.  s: survivor (pending after the fill phase), d: dead slot, f: finished in the
    fill phase."""
    for n in (1, 63, 64, 65, 127, 128, 129):
        t = Q.trace(Q.layout_live(n))
        assert t["machine_lanes"] == Q.machine_steps_of(n) and t["max_pending"] == min(n, 64), (n, t)
    t = Q.trace(Q.LAYOUTS["63_pending_then_64"])
    assert t["max_pending"] == 127 and t["machine_lanes"] == [64, 63]
    t = Q.trace(Q.LAYOUTS["dead_batch_between"])
    assert t["fills"] == 3 and t["machine_lanes"] == [64, 6]
    t = Q.trace(Q.LAYOUTS["63_of_64_dead"])
    assert t["machine_lanes"] == [1]
    t = Q.trace(Q.LAYOUTS["all_finished_in_fill"])
    assert t["machine_lanes"] == [] and t["fills"] == 2
    t = Q.trace(Q.LAYOUTS["partial_last_batch"])
    assert t["machine_lanes"] == [64, 36] and t["last_got"] == 37
    # the group of 256 slots every wave of a one-workgroup launch draws at a time (n >= 8192): the same states whichever wave draws it
    t = Q.trace(Q.GROUP_256)
    assert t["max_pending"] == 127 and t["machine_lanes"] == [64, 64] and t["fills"] == 4 and t["left"] == 0
    big = Q.half_dead_reservations(4096 + 37)
    assert len(big) == 4096 + 37 and (np.array(list(big)) == "d").sum() == 32 * 32
    assert all(set(big[k:k + 64]) == {"s"} for k in range(0, 4096, 128)) and all(big[k + 32:k + 64] == "d" * 32 for k in range(64, 4096, 128))

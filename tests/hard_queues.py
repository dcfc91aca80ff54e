"""Queue layouts of the hard-ray stage tests (test_gpu_stages_hard.py) and a model of what a wave of k_hard_shadow / k_hard_path makes
of them (acn_k_hard.h: the pending list).  A layout is a string, one letter per slot of the queue:
    s   a record that is pending after the fill phase: one with a resume word, or a probe a machine element is left for
    f   a probe the fill phase finishes (an in-line element occludes it, or no machine element survives the pre-tests)
    d   a dead slot (pixel 0xFFFFFFFF)
A wave takes 64 consecutive slots per fill step, fills while fewer than 64 indices are pending and input remains, and then runs the
machine phase on up to 64 of them.  Which wave of a launch draws which slots is not decided by the test -- except that with ONE
workgroup and 8192 <= n < 10240 records every wave draws 256 consecutive, 256-aligned slots at a time (balanced_batch), so a layout
made of 256-slot groups that leave nothing pending shows every wave the same sequence of list states."""

GROUP_256 = "s" * 63 + "d" + "s" * 64 + "d" * 64 + "d" * 63 + "s"
GROUPS = 32                                   # x 256 = 8192 slots

LAYOUTS = {
    "63_pending_then_64": "s" * 63 + "d" + "s" * 64,
    "dead_batch_between": "s" * 35 + "d" * 29 + "d" * 64 + "s" * 35 + "d" * 29,
    "63_of_64_dead": "d" * 40 + "s" + "d" * 23,
    "all_finished_in_fill": "f" * 64 + "f" * 30 + "d" * 5,
    "partial_last_batch": "s" * 64 + "s" * 36 + "f",
}


def layout_live(n):
    return "s" * n


def machine_steps_of(n):
    return [64] * (n // 64) + ([n % 64] if n % 64 else [])


def half_dead_reservations(n):
    """every second reservation of 64 slots half dead"""
    out = ""
    k = 0
    while len(out) < n:
        out += "s" * 64 if k % 2 == 0 else "s" * 32 + "d" * 32
        k += 1
    return out[:n]


def trace(layout):
    """one wave working the whole layout off: the lanes of its machine steps, the most its list held, its fill steps"""
    pending, pos, fills, most, last_got = 0, 0, 0, 0, None
    machine = []
    more = True
    while True:
        while pending < 64 and more:
            got = min(64, len(layout) - pos)
            if got == 0:
                more = False
                break
            pending += layout[pos:pos + got].count("s")
            pos += got
            fills += 1
            last_got = got
            most = max(most, pending)
            assert pending <= 127
        if pending == 0:
            break
        take = min(64, pending)
        pending -= take
        machine.append(take)
    return {"machine_lanes": machine, "max_pending": most, "fills": fills, "last_got": last_got, "left": pending}

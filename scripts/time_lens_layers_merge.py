#!/usr/bin/env python3
"""What the layered merge costs per byte beside the statistics merge.

    python scripts/time_lens_layers_merge.py [--width 1920 --height 1080] [--steps 7] [--out profiles/r13/lens_layers_merge.json]

n = width x height positions, a null index, no EMPTY record on either side: the planes are synthetic -- per position two layers of
two classes and a rest on both sides, the part's layers in the accumulator's order on even positions and crossed on odd ones, so every
lane runs both pair merges.  In one process, after a warm-up of each, alternating --steps times between two synchronisations:
  layers_merge    acn_lens_layers_merge_dev      896 bytes read, 448 written per position
  stats_merge     acn_lens_stats_merge_dev       128 bytes read,  64 written per record, on the same n
  layers_resolve  acn_lens_layers_resolve_dev    192 bytes read, 40 written (colour, noise)
The accumulators are restored from a copy before every timed call (outside the clock), so every run merges the same records.
Prints one JSON line: the times and the time per byte moved of either merge."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    n = args.width * args.height
    h = A.Handle(A.Scene.build("wine_glass", image_width=64, image_height=36, path_samples=4, direct_samples=12).flatten())
    dev = torch.device("cuda", h.device)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, generator=g, dtype=torch.float64, device=dev)

    def side(crossed):
        surf, st = rnd(2, n, 16) + 0.5, rnd(3, n, 8)
        odd = (torch.arange(n, device=dev) % 2 == 1) & crossed
        for l in range(2):
            e = torch.where(odd, torch.full((n,), 1.0 - l, dtype=torch.float64, device=dev), torch.full((n,), float(l), dtype=torch.float64, device=dev))
            surf[l, :, 7], surf[l, :, 8], surf[l, :, 12], surf[l, :, 13] = 5.0 + 2.0 * e, -1.0, 2.0, 0.0
        st[:, :, 0] = torch.tensor([9.0, 5.0, 2.0], dtype=torch.float64, device=dev)[:, None]
        st[:, :, 7] = 0.0
        return surf.contiguous(), st.contiguous()

    acc0_surf, acc0_st = side(False)
    part_surf, part_st = side(True)
    d_acc_surf, d_acc_st = acc0_surf.clone(), acc0_st.clone()
    d_acc1, part1 = acc0_st[0].clone(), part_st[0].contiguous()
    d_rgb, d_noise = torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n,), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def restore():
        d_acc_surf.copy_(acc0_surf); d_acc_st.copy_(acc0_st); d_acc1.copy_(acc0_st[0])

    calls = {
        "layers_merge": lambda: h.lens_layers_merge_dev(d_acc_surf.data_ptr(), d_acc_st.data_ptr(), n, part_surf.data_ptr(), part_st.data_ptr(), n, None, stream=stream),
        "stats_merge": lambda: h.lens_stats_merge_dev(d_acc1.data_ptr(), n, part1.data_ptr(), n, None, stream=stream),
        "layers_resolve": lambda: h.lens_layers_resolve_dev(d_acc_st.data_ptr(), n, d_rgb.data_ptr(), d_noise.data_ptr(), None, stream=stream),
    }

    def timed(f):
        restore()
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for f in calls.values():
        timed(f)
    times = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, f in calls.items():
            times[name].append(timed(f))
    restore()
    calls["layers_merge"]()
    torch.cuda.synchronize()
    merged_all = bool((d_acc_st[0, :, 0] + d_acc_st[1, :, 0] == 28.0).all() and (d_acc_st[2, :, 0] == 4.0).all())   # (nothing was demoted)
    h.close()
    med = {name: float(np.median(v)) for name, v in times.items()}
    bytes_moved = {"layers_merge": 1344 * n, "stats_merge": 192 * n}
    ns_per_byte = {name: med[name] * 1e6 / bytes_moved[name] for name in bytes_moved}
    res = {"positions": n, "steps": args.steps,
           "ms": {name: {"median": med[name], "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 4) for x in v]} for name, v in times.items()},
           "bytes_moved": bytes_moved, "ns_per_byte": ns_per_byte, "GB_per_s": {name: bytes_moved[name] / (med[name] * 1e6) for name in bytes_moved},
           "layers_over_stats_per_byte": ns_per_byte["layers_merge"] / ns_per_byte["stats_merge"], "every_position_ran_both_pair_merges": merged_all}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

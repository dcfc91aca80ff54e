#!/usr/bin/env python3
"""Device time of acn_denoise_dev.

    python scripts/time_denoise.py [--steps 12] [--out profiles/r05/denoise_times.json] [--bench-ms MS]

Two frames of wine_glass rendered at p8 / d16 with their FOLLOW records, device-resident: 1920x1080 (bench.py's frame) and
3840x2160.  denoise_dev runs on the caller's stream between two HIP events; per iteration count 1 .. 5 the median of --steps
runs after three warm-up runs.  The time of level i is the difference between the calls with i + 1 and i levels (the last level
of a call also remodulates and writes the frame, so the differences are those of inner levels); the call with one level is
prepare + variance + that last level.  Next to it stands the frame the filter is meant to replace, timed the same way: the
1080p main pass at p64 / d200 (acn_render_main_pass_dev, what bench.py measures), and the p8 / d16 main pass and FOLLOW call
the filtered frame costs.  --bench-ms: bench.py's own figure for the p64 / d200 frame on the same machine, recorded as given.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-ms", type=float, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A

    stream = torch.cuda.current_stream().cuda_stream

    def event_ms(call, runs):
        out = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    def stats(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    res = {"steps": args.steps, "frames": {}}
    for w, hh in ((1920, 1080), (3840, 2160)):
        n = w * hh
        build = lambda p, d: A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=p, direct_samples=d).flatten()
        h = A.Handle(build(8, 16))
        pos = torch.from_numpy(A.main_pass_positions(w, hh)).to("cuda")
        lin = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        rec = torch.empty((n, 16), dtype=torch.float64, device="cuda")
        out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        render = lambda: h.render_main_pass_dev(0, n, lin.data_ptr(), linear=True, stream=stream)
        follow = lambda: h.surface_positions_dev(pos.data_ptr(), n, rec.data_ptr(), follow=True, stream=stream)
        event_ms(render, 2), event_ms(follow, 2)
        fr = {"pixels": n, "render_p8_d16_ms": stats(event_ms(render, args.steps)), "follow_records_ms": stats(event_ms(follow, args.steps))}
        calls = {}
        for it in (1, 2, 3, 4, 5):
            call = lambda it=it: h.denoise_dev(lin.data_ptr(), rec.data_ptr(), w, hh, out.data_ptr(), stream=stream, iterations=it)
            event_ms(call, 3)
            calls[it] = stats(event_ms(call, args.steps))
        fr["denoise_ms_by_iterations"] = calls
        fr["denoise_default_ms"] = calls[5]["median"]
        fr["prepare_variance_last_level_ms"] = calls[1]["median"]
        fr["level_ms"] = {f"stride_{1 << (it - 1)}": calls[it + 1]["median"] - calls[it]["median"] for it in (1, 2, 3, 4)}
        fr["scratch_bytes"] = 128 * n
        frac = float((rec[:, 0] < float("inf")).double().mean())
        fr["hit_fraction"] = frac
        h.close()
        if (w, hh) == (1920, 1080):
            h64 = A.Handle(build(64, 200))
            full = lambda: h64.render_main_pass_dev(0, n, lin.data_ptr(), linear=True, stream=stream)
            event_ms(full, 2)
            fr["render_p64_d200_ms"] = stats(event_ms(full, args.steps))
            h64.close()
            fr["denoise_over_p64_d200_frame"] = fr["denoise_default_ms"] / fr["render_p64_d200_ms"]["median"]
            fr["filtered_p8_frame_over_p64_d200_frame"] = (fr["render_p8_d16_ms"]["median"] + fr["follow_records_ms"]["median"]
                                                           + fr["denoise_default_ms"]) / fr["render_p64_d200_ms"]["median"]
            if args.bench_ms is not None:
                fr["bench_py_p64_d200_ms"] = args.bench_ms
        res["frames"][f"{w}x{hh}"] = fr
        del pos, lin, rec, out
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

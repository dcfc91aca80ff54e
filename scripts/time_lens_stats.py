#!/usr/bin/env python3
"""What the lens sample statistics cost.

    python scripts/time_lens_stats.py [--steps 5] [--samples 16] [--width 1920 --height 1080] [--parent-libdir DIR]
                                      [--out profiles/r06/lens_stats_times.json]

Frame: wine_glass at p4 / d12, K jittered lens rays per pixel.  In one process, after one warm-up of each, alternating --steps times:
  lens        acn_render_lens_main_pass_dev( 0, n, linear )                          the call without statistics
  lens_stats  acn_render_lens_stats_main_pass_dev( 0, n, linear, d_rgb, d_stats )    the same frame and its records
  merge       acn_lens_stats_merge_dev of the frame's records into an accumulator that holds records already
  resolve     acn_lens_stats_resolve_dev, colour and noise
  denoise     acn_denoise_dev on the mean            denoise_stats   acn_denoise_stats_dev on the records
--parent-libdir: a build of the commit before the statistics existed (ACN_LIBDIR).  `lens` is then also timed there, in child
processes that alternate with child processes of this build, a fresh process each, --steps frames per process.
Everything runs on torch's current stream and ends in a synchronise; a host clock is taken around each.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    import numpy as np
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [round(x, 3) for x in v]}


def timed(f):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def child(args):
    """`lens` alone, --steps times after a warm-up: one JSON list of ms"""
    import torch
    import actinon_amd as A
    w, hh, K = args.width, args.height, args.samples
    n = w * hh
    h = A.Handle(A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=4, direct_samples=12).flatten())
    stream = torch.cuda.current_stream().cuda_stream
    d_rgb = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    lens = lambda: h.render_lens_main_pass_dev(0, n, d_rgb.data_ptr(), linear=True, stream=stream, samples=K, jitter=True)
    timed(lens)
    print(json.dumps([timed(lens) for _ in range(args.steps)]), flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent-libdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"frame": f"wine_glass {args.width}x{args.height} p4 d12", "samples": args.samples, "steps": args.steps}
    if args.parent_libdir:                                    # before this process opens the GPU: one process at a time
        runs = {"parent": [], "this": []}
        for _ in range(2):
            for name, libdir in (("parent", os.path.abspath(args.parent_libdir)), ("this", "")):
                env = dict(os.environ, ACN_LIBDIR=libdir)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--samples", str(args.samples),
                                    "--width", str(args.width), "--height", str(args.height)], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"child process ({name}) failed with {r.returncode}:\n{r.stdout}{r.stderr}")
                runs[name] += json.loads(r.stdout.strip().splitlines()[-1])
        res["lens_ms_parent_build"] = stats(runs["parent"])
        res["lens_ms_this_build_child"] = stats(runs["this"])
    import numpy as np
    import torch
    import actinon_amd as A

    w, hh, K = args.width, args.height, args.samples
    n = w * hh
    flat = A.Scene.build("wine_glass", image_width=w, image_height=hh, path_samples=4, direct_samples=12).flatten()
    h = A.Handle(flat)
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(dev)
    d_rgb = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_rgb2 = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_stats = torch.empty((n, 8), dtype=torch.float64, device=dev)
    d_acc = torch.empty((n, 8), dtype=torch.float64, device=dev)
    d_noise = torch.empty((n,), dtype=torch.float64, device=dev)
    d_surf = torch.empty((n, 16), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr(), follow=True)
    lens_kw = dict(samples=K, jitter=True)
    retries = {"lens": 0, "lens_stats": 0}

    def lens():
        h.render_lens_main_pass_dev(0, n, d_rgb.data_ptr(), linear=True, stream=stream, **lens_kw)
        retries["lens"] += int(h.last_stages()["retries"])

    def lens_stats():
        h.render_lens_stats_main_pass_dev(0, n, d_rgb2.data_ptr(), d_stats.data_ptr(), linear=True, stream=stream, **lens_kw)
        retries["lens_stats"] += int(h.last_stages()["retries"])

    calls = {
        "lens": lens, "lens_stats": lens_stats,
        "merge": lambda: h.lens_stats_merge_dev(d_acc.data_ptr(), n, d_stats.data_ptr(), n, None, stream=stream),
        "resolve": lambda: h.lens_stats_resolve_dev(d_acc.data_ptr(), n, d_out.data_ptr(), d_noise.data_ptr(), stream=stream),
        "denoise": lambda: h.denoise_dev(d_rgb.data_ptr(), d_surf.data_ptr(), w, hh, d_out.data_ptr(), stream=stream),
        "denoise_stats": lambda: h.denoise_stats_dev(d_stats.data_ptr(), d_surf.data_ptr(), w, hh, d_out.data_ptr(), stream=stream),
    }
    timed(lens), timed(lens_stats)                            # warm-up: code objects, lanes, learned rates, slice buffers
    d_acc.copy_(d_stats)
    for name in ("merge", "resolve", "denoise", "denoise_stats"):
        timed(calls[name])
    times = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, f in calls.items():
            times[name].append(timed(f))
    same = bool(torch.equal(d_rgb, d_rgb2)) and bool(torch.equal(d_stats[:, 1:4], d_rgb))
    h.close()
    res.update({name + "_ms": stats(v) for name, v in times.items()})
    res.update({"lens_stats_over_lens": float(np.median(times["lens_stats"]) / np.median(times["lens"])),
                "denoise_stats_over_denoise": float(np.median(times["denoise_stats"]) / np.median(times["denoise"])),
                "retries": retries, "same_frame_bits": same,
                "radiance_bytes_of_a_slice_read_twice": 24 * K * min(n, max((1 << 21) // K, 1)), "record_bytes": 64 * n})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

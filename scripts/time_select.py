#!/usr/bin/env python3
"""What selecting the pixels of a pass costs.

    python scripts/time_select.py [--width 1920 --height 1080] [--selected 0.1] [--calls 50] [--runs 7] [--out profiles/r07/select_times.json]

Keys: n = width * height uniform doubles in [ 0, 1 ), threshold 1 - selected, so that `selected` of them lie above it.  On one handle
(a small scene: the select calls do not look at it), after a warm-up of each, --runs times, alternating:
  select     acn_select_above_dev: indices and raster positions, the count returned to the host (the call's one synchronisation)
  histogram  acn_key_histogram_dev on the handle's stream (the call waits)
  torch      what tools/render_progressive.py did before: torch.nonzero, the centres of the pixels by a torch.stack, and the
             int( idx.numel() ) that the tool needs -- the path the select call replaces
A run is --calls calls between two synchronisations under a host clock; the figure is the run's time per call.  Prints one JSON line
with the median and the spread of every figure, and checks once that the three agree on what is selected."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    import numpy as np
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2),
            "runs_us": [round(x, 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--selected", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    import render_progressive as tool
    if A.device_count() < 1:
        sys.exit("no HIP device: a time is a time on the GPU")
    w, hh = args.width, args.height
    n = w * hh
    h = A.Handle(A.Scene.build("wine_glass", image_width=64, image_height=36, path_samples=4, direct_samples=12).flatten())
    dev = torch.device("cuda", h.device)
    key = np.random.default_rng(7).random(n)
    threshold = 1.0 - args.selected
    d_key = torch.from_numpy(key).to(dev)
    d_idx = torch.empty((n,), dtype=torch.int64, device=dev)
    d_pos = torch.empty((n, 2), dtype=torch.float64, device=dev)
    d_hist = torch.empty((A.abi.ACN_KEY_HIST_WORDS,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def select():
        return h.select_above_dev(d_key.data_ptr(), n, threshold, n, d_index_ptr=d_idx.data_ptr(), d_pos_ptr=d_pos.data_ptr(), raster_width=w)

    def histogram():
        h.key_histogram_dev(d_key.data_ptr(), n, d_hist.data_ptr())

    def with_torch():
        idx = tool.select(d_key, threshold)
        m = int(idx.numel())
        return idx, tool.centres(idx, w), m

    # once: the three agree
    m = select()
    idx, pos, m_t = with_torch()
    histogram()
    torch.cuda.synchronize(dev)
    assert m == m_t == int((key > threshold).sum()) and torch.equal(d_idx[:m], idx) and torch.equal(d_pos[:m], pos)
    assert int(d_hist.sum().item()) == n
    variants = {"select": select, "histogram": histogram, "torch": with_torch}
    for f in variants.values():
        for _ in range(10):
            f()
    times = {name: [] for name in variants}
    for _ in range(args.runs):
        for name, f in variants.items():
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            for _ in range(args.calls):
                f()
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t) * 1e6 / args.calls)
    h.close()
    result = {"n": n, "width": w, "height": hh, "selected": m, "calls_per_run": args.calls, "runs": args.runs,
              "device": torch.cuda.get_device_name(dev), **{name: stats(v) for name, v in times.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

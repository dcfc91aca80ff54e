#!/usr/bin/env python3
"""Ray calls against position calls.

    python scripts/time_rays.py [--steps 10] [--pano 2048x1024]

bench.py's frame (wine_glass 1920x1080 p64 d200) on one handle: acn_render_rays_dev of the frame's own camera rays against
acn_render_main_pass_dev, warm, interleaved step by step, every call on the caller's stream and timed by the host clock
between two device synchronisations; both must give the same bits.  Then an equirectangular panorama of the same scene
from its camera (actinon_amd.cameras.panorama_rays) on the same handle.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--pano", default="2048x1024")
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd.cameras import panorama_rays

    W, H = 1920, 1080
    flat = A.Scene.build("wine_glass", image_width=W, image_height=H, path_samples=64, direct_samples=200).flatten()
    S = int(flat.params.path_samples)
    n = W * H
    h = A.Handle(flat)
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.from_numpy(A.main_pass_positions(W, H)).to("cuda")
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    h.camera_rays_dev(pos.data_ptr(), n, rays.data_ptr(), stream=stream)
    out_pos = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    out_rays = torch.empty_like(out_pos)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, h.last_stages()

    def main_pass():
        h.render_main_pass_dev(0, n, out_pos.data_ptr(), linear=True, stream=stream)

    def ray_call():
        h.render_rays_dev(rays.data_ptr(), n, out_rays.data_ptr(), linear=True, stream=stream)

    for _ in range(2):
        timed(main_pass)
        timed(ray_call)
    t_pos, t_rays, retries = [], [], 0
    for _ in range(args.steps):
        for call, into in ((main_pass, t_pos), (ray_call, t_rays)):
            ms, st = timed(call)
            into.append(ms)
            retries += int(st["retries"])
    same = bool(torch.equal(out_pos, out_rays))

    pw, ph = (int(v) for v in args.pano.lower().split("x"))
    prm = flat.params
    prays = torch.from_numpy(panorama_rays(prm.camera_position[:], prm.camera_view_direction[:], prm.camera_top_direction[:],
                                           pw, ph)).to("cuda")
    pout = torch.empty((pw * ph, 3), dtype=torch.float64, device="cuda")

    def pano():
        h.render_rays_dev(prays.data_ptr(), pw * ph, pout.data_ptr(), linear=True, stream=stream)

    timed(pano)
    t_pano = []
    for _ in range(3):
        ms, st = timed(pano)
        t_pano.append(ms)
        retries += int(st["retries"])
    h.close()
    med = lambda v: float(np.median(v))
    print(json.dumps({
        "frame": f"wine_glass {W}x{H} p{S} d{int(prm.direct_samples)}, one handle, default lanes, linear output",
        "steps": args.steps,
        "main_pass_ms": {"median": med(t_pos), "min": min(t_pos), "max": max(t_pos)},
        "rays_ms": {"median": med(t_rays), "min": min(t_rays), "max": max(t_rays)},
        "rays_over_main_pass": med(t_rays) / med(t_pos),
        "same_bits": same,
        "retries": retries,
        "panorama": {"size": f"{pw}x{ph}", "ms": {"median": med(t_pano), "min": min(t_pano)},
                     "msamples_per_s": pw * ph * S / (med(t_pano) * 1e-3) / 1e6},
    }), flush=True)


if __name__ == "__main__":
    main()

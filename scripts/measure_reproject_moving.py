#!/usr/bin/env python3
"""What the history is worth on an object that turns.

    python scripts/measure_reproject_moving.py [--frames 8] [--degrees 2] [--samples 4] [--ref-samples 256] [--element 1] [--axis 0,0,1]
                                               [--moved-max-history 8] [--all-kinds] [--out profiles/r18/reproject_moving_quality.json]

Frame: wine_glass as its script sets it (400 x 400, p500 / d200); the camera stays, and root element --element of the scene's matter
(1: the glass) turns --degrees per frame about --axis through its own position (actinon_amd.motion.rigid_copy, acn_scene_replace).
Every frame renders K = --samples jittered samples per pixel with their statistics (seed = frame) and first-hit surface records; from
frame 1 on the history of the frame before is pooled with them (acn_lens_stats_merge_dev) twice, side by side on the same samples:
  at_rest   acn_reproject_dev: the world taken to be at rest
  moving    acn_reproject_moving_dev with the table of acn_motion_from_scenes( previous scene, this scene, --moved-max-history )
For the LAST frame, against a converged frame of its scene (--ref-samples jittered samples, seed 99), the linear RMSE of raw (the
frame's own K samples), at_rest and moving over the pixels that show the turned object, and over all pixels; and how many of those
pixels took a history either way.  --all-kinds: reject_kinds = 0, history on glass and mirrors too (the default mask takes none on a
Fresnel or transparent surface, whichever call).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before torch initialises HIP (the library's concurrent lanes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--degrees", type=float, default=2.0)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--ref-samples", type=int, default=256)
    ap.add_argument("--element", type=int, default=1)
    ap.add_argument("--axis", default="0,0,1")
    ap.add_argument("--moved-max-history", type=float, default=8.0)
    ap.add_argument("--all-kinds", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd import abi
    from actinon_amd.motion import rigid_copy, rotation_about, subtree

    flat = A.Scene.build("wine_glass").flatten()
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n, K = w * hh, args.samples
    node = flat.elems_of(flat.c.matter_root)[args.element]
    axis = tuple(float(v) for v in args.axis.split(","))
    members = np.array(sorted(i for i, _ in subtree(flat, node)))
    params = dict(reject_kinds=0) if args.all_kinds else {}
    h = A.Handle(flat)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", h.device))
    new = lambda *shape: torch.zeros(shape, **f64)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(f64["device"])
    d_surf, d_prev_surf, d_cur = new(n, 16), new(n, 16), new(n, 8)
    acc = {v: new(n, 8) for v in ("at_rest", "moving")}
    prev = {v: new(n, 8) for v in acc}
    torch.cuda.synchronize()
    prev_params, prev_flat, per_frame = None, flat, []
    took = {v: torch.zeros(n, dtype=torch.bool, device=f64["device"]) for v in acc}
    for f in range(args.frames):
        cur_flat = rigid_copy(flat, node, rotation_about(axis, args.degrees * f), pivot=list(flat.node(node).pos)) if f else flat
        if f:
            h.replace(cur_flat)
        h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
        h.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, samples=K, jitter=True, seed=f)
        if f:
            table, report = A.motion_from_scenes(prev_flat, cur_flat, args.moved_max_history)
            d_table = torch.from_numpy(table).to(f64["device"])
            h.reproject_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), prev["at_rest"].data_ptr(), acc["at_rest"].data_ptr(), **params)
            h.reproject_moving_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), prev["moving"].data_ptr(), d_table.data_ptr(), len(table),
                                   acc["moving"].data_ptr(), **params)
            for v in acc:
                took[v] = acc[v][:, 0] >= 1
                h.lens_stats_merge_dev(acc[v].data_ptr(), n, d_cur.data_ptr(), n)
        else:
            report = None
            for v in acc:
                acc[v].copy_(d_cur)
            torch.cuda.synchronize()
        per_frame.append({"frame": f, "table": report, **{f"with_history_{v}": float(took[v].double().mean()) for v in acc},
                          **{f"mean_n_{v}": float(acc[v][:, 0].mean()) for v in acc}})
        print(per_frame[-1], file=sys.stderr, flush=True)
        prev_params = abi.Params()
        C.memmove(C.addressof(prev_params), C.addressof(h.params), C.sizeof(abi.Params))
        prev_flat = cur_flat
        if f < args.frames - 1:
            d_surf, d_prev_surf = d_prev_surf, d_surf
            for v in acc:
                acc[v], prev[v] = prev[v], acc[v]
    surf = d_surf.cpu().numpy()
    obj = np.where(surf[:, 7] >= 0, surf[:, 7], surf[:, 8]).astype(np.int64)
    on_object = np.isfinite(surf[:, 0]) & np.isin(obj, members)
    frames = {"raw": d_cur[:, 1:4].cpu().numpy(), "at_rest": acc["at_rest"][:, 1:4].cpu().numpy(), "moving": acc["moving"][:, 1:4].cpu().numpy()}
    took = {v: t.cpu().numpy() for v, t in took.items()}
    res = {"scene": f"wine_glass {w}x{hh} p{flat.params.path_samples} d{flat.params.direct_samples}", "frames": args.frames, "degrees_per_frame": args.degrees,
           "axis": axis, "element": args.element, "node": int(node), "samples": K, "ref_samples": args.ref_samples, "moved_max_history": args.moved_max_history,
           "reject_kinds": 0 if args.all_kinds else abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS, "pixels": n, "pixels_on_the_object": int(on_object.sum()),
           "with_history_on_the_object_last_frame": {v: float(took[v][on_object].mean()) for v in took}, "per_frame": per_frame,
           "learning_passes": h.info()["learning_passes"], "replaces": h.info()["replaces"]}
    if args.ref_samples:
        ref = np.empty((n, 3))
        block = 16384
        d_ref = torch.empty((block, 3), **f64)
        for first in range(0, n, block):
            cnt = min(block, n - first)
            h.render_lens_main_pass_dev(first, cnt, d_ref.data_ptr(), linear=True, samples=args.ref_samples, jitter=True, seed=99)
            ref[first:first + cnt] = d_ref[:cnt].cpu().numpy()
            print(f"reference: {first + cnt} of {n} pixels", file=sys.stderr, flush=True)
        for label, mask in (("on_the_object", on_object), ("all", np.ones(n, bool))):
            for name, img in frames.items():
                d = img[mask] - ref[mask]
                res.setdefault("rmse_linear", {}).setdefault(label, {})[name] = float(np.sqrt(np.mean(d * d)))
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the shadow guard is worth where a moving object's shadow crosses the floor.

    python scripts/measure_shadow_history.py [--frames 8] [--shift=-0.12,0,0] [--samples 4] [--ref-samples 256] [--element 1] [--shadow-samples 16]
                                             [--tolerance 0.25] [--drop] [--orbit-frames 4 --orbit-deg 2] [--out profiles/r24/shadow_history.json]

Frame: primitives as its script sets it (400 x 400, p30 / d30); the camera stays, and root element --element of the scene's matter
(1: the sphere) is shifted by --shift per frame over the floor (actinon_amd.motion.rigid_copy, acn_scene_replace).  Every frame renders
K = --samples jittered samples per pixel with their statistics (seed = frame), first-hit surface records and shadow records; from frame
1 on the history of the frame before is pooled with them twice, side by side on the same samples:
  moving    acn_reproject_moving_dev with the table of acn_motion_from_scenes: the library before the guard
  guarded   the same, then acn_shadow_limit_history_dev (S = --shadow-samples) between reproject and merge
The floor of this scene is polished (a Fresnel surface), which the default reject_kinds takes no history on: both variants run with
ACN_SURF_FRESNEL taken out of the mask, as tools/render_turntable.py --allow-fresnel does.
For the LAST frame, against a converged frame of its scene (--ref-samples jittered samples, seed 99), the linear RMSE of raw (the
frame's own K samples), moving and guarded over the CHANGED pixels -- those whose S = 64 shadow share differs between the last two
frames by more than 0.25 -- and over all pixels.
Then the false-positive rate of the tolerance: on the scene at rest the camera orbits --orbit-deg per frame for --orbit-frames frames
(acn_reproject_dev), and per frame the share of the history-carrying pixels the guard limits is recorded.  Prints one JSON line."""
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
    ap.add_argument("--shift", default="-0.12,0,0")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--ref-samples", type=int, default=256)
    ap.add_argument("--element", type=int, default=1)
    ap.add_argument("--shadow-samples", type=int, default=16)
    ap.add_argument("--tolerance", type=float, default=None)
    ap.add_argument("--drop", action="store_true")
    ap.add_argument("--orbit-frames", type=int, default=4)
    ap.add_argument("--orbit-deg", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import actinon_amd as A
    from actinon_amd import abi
    from actinon_amd.cameras import orbit_camera
    from actinon_amd.motion import rigid_copy

    flat = A.Scene.build("primitives").flatten()
    w, hh = int(flat.params.image_width), int(flat.params.image_height)
    n, K = w * hh, args.samples
    node = flat.elems_of(flat.c.matter_root)[args.element]
    shift = tuple(float(v) for v in args.shift.split(","))
    tol = abi.ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE if args.tolerance is None else args.tolerance
    params = dict(reject_kinds=abi.ACN_REPROJECT_DEFAULT_REJECT_KINDS & ~abi.ACN_SURF_FRESNEL)
    guard = dict(tolerance=args.tolerance, drop=args.drop)
    h = A.Handle(flat)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda", h.device))
    new = lambda *shape: torch.zeros(shape, **f64)
    d_pos = torch.from_numpy(A.main_pass_positions(w, hh)).to(f64["device"])
    d_surf, d_prev_surf, d_cur = new(n, 16), new(n, 16), new(n, 8)
    d_shadow, d_prev_shadow, d_motion, d_change = new(n, 16), new(n, 16), new(n, 2), new(n)
    d_share64 = [new(n, 16), new(n, 16)]
    acc = {v: new(n, 8) for v in ("moving", "guarded")}
    prev = {v: new(n, 8) for v in acc}
    torch.cuda.synchronize()

    def keep_params():
        p = abi.Params()
        C.memmove(C.addressof(p), C.addressof(h.params), C.sizeof(abi.Params))
        return p

    prev_params, prev_flat, per_frame = None, flat, []
    for f in range(args.frames):
        cur_flat = rigid_copy(flat, node, shift=[s * f for s in shift]) if f else flat
        if f:
            h.replace(cur_flat)
        h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
        h.shadow_records_dev(d_surf.data_ptr(), n, d_shadow.data_ptr(), samples=args.shadow_samples)
        if f >= args.frames - 2:
            h.shadow_records_dev(d_surf.data_ptr(), n, d_share64[f - (args.frames - 2)].data_ptr(), samples=64)
        h.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, samples=K, jitter=True, seed=f)
        row = {"frame": f}
        if f:
            table, report = A.motion_from_scenes(prev_flat, cur_flat)
            d_table = torch.from_numpy(table).to(f64["device"])
            for v in acc:
                h.reproject_moving_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), prev[v].data_ptr(), d_table.data_ptr(), len(table),
                                       acc[v].data_ptr(), d_motion.data_ptr(), **params)
                row[f"with_history_{v}"] = float((acc[v][:, 0] >= 1).double().mean())
                if v == "guarded":
                    h.shadow_limit_history_dev(acc[v].data_ptr(), d_motion.data_ptr(), d_shadow.data_ptr(), d_prev_shadow.data_ptr(), n, w, hh,
                                               d_change.data_ptr(), **guard)
                    row["limited_of_the_histories"] = float((d_change > tol).double().sum()) / max(1.0, float((d_change == d_change).double().sum()))
                h.lens_stats_merge_dev(acc[v].data_ptr(), n, d_cur.data_ptr(), n)
                row[f"mean_n_{v}"] = float(acc[v][:, 0].mean())
        else:
            for v in acc:
                acc[v].copy_(d_cur)
            torch.cuda.synchronize()
        per_frame.append(row)
        print(row, file=sys.stderr, flush=True)
        prev_params, prev_flat = keep_params(), cur_flat
        if f < args.frames - 1:
            d_surf, d_prev_surf = d_prev_surf, d_surf
            d_shadow, d_prev_shadow = d_prev_shadow, d_shadow
            for v in acc:
                acc[v], prev[v] = prev[v], acc[v]
    share = [d[:, 5].cpu().numpy() for d in d_share64]
    state = [d[:, 0].cpu().numpy() for d in d_share64]
    changed = (state[0] == 1) & (state[1] == 1) & (np.abs(share[1] - share[0]) > 0.25)
    frames = {"raw": d_cur[:, 1:4].cpu().numpy(), "moving": acc["moving"][:, 1:4].cpu().numpy(), "guarded": acc["guarded"][:, 1:4].cpu().numpy()}
    res = {"scene": f"primitives {w}x{hh} p{flat.params.path_samples} d{flat.params.direct_samples}", "frames": args.frames, "shift_per_frame": shift,
           "element": args.element, "node": int(node), "samples": K, "ref_samples": args.ref_samples, "shadow_samples": args.shadow_samples,
           "tolerance": tol, "drop": bool(args.drop), "reject_kinds": params["reject_kinds"], "pixels": n, "changed_pixels": int(changed.sum()),
           "per_frame": per_frame}
    if args.ref_samples:
        ref = np.empty((n, 3))
        block = 16384
        d_ref = torch.empty((block, 3), **f64)
        for first in range(0, n, block):
            cnt = min(block, n - first)
            h.render_lens_main_pass_dev(first, cnt, d_ref.data_ptr(), linear=True, samples=args.ref_samples, jitter=True, seed=99)
            ref[first:first + cnt] = d_ref[:cnt].cpu().numpy()
            print(f"reference: {first + cnt} of {n} pixels", file=sys.stderr, flush=True)
        for label, mask in (("changed", changed), ("all", np.ones(n, bool))):
            for name, img in frames.items():
                d = img[mask] - ref[mask]
                res.setdefault("rmse_linear", {}).setdefault(label, {})[name] = float(np.sqrt(np.mean(d * d))) if mask.any() else None

    # the tolerance's false positives: nothing moves, the camera orbits
    h.replace(flat)
    orbit = []
    for f in range(args.orbit_frames + 1):
        if f:
            h.set_params(**orbit_camera(flat.params, args.orbit_deg * f))
        h.surface_positions_dev(d_pos.data_ptr(), n, d_surf.data_ptr())
        h.shadow_records_dev(d_surf.data_ptr(), n, d_shadow.data_ptr(), samples=args.shadow_samples)
        h.render_lens_stats_main_pass_dev(0, n, None, d_cur.data_ptr(), linear=True, samples=K, jitter=True, seed=f)
        if f:
            a = acc["guarded"]
            h.reproject_dev(d_surf.data_ptr(), n, prev_params, d_prev_surf.data_ptr(), prev["guarded"].data_ptr(), a.data_ptr(), d_motion.data_ptr(), **params)
            carrying = float((a[:, 0] >= 1).double().sum())
            h.shadow_limit_history_dev(a.data_ptr(), d_motion.data_ptr(), d_shadow.data_ptr(), d_prev_shadow.data_ptr(), n, w, hh, d_change.data_ptr(), **guard)
            limited = float((d_change > tol).double().sum())
            orbit.append({"frame": f, "history_carrying_pixels": int(carrying), "limited": int(limited), "share": limited / max(1.0, carrying)})
            h.lens_stats_merge_dev(a.data_ptr(), n, d_cur.data_ptr(), n)
        else:
            acc["guarded"].copy_(d_cur)
            torch.cuda.synchronize()
        prev_params = keep_params()
        d_surf, d_prev_surf = d_prev_surf, d_surf
        d_shadow, d_prev_shadow = d_prev_shadow, d_shadow
        acc["guarded"], prev["guarded"] = prev["guarded"], acc["guarded"]
    res["orbit_at_rest"] = {"degrees_per_frame": args.orbit_deg, "per_frame": orbit,
                            "share_limited": float(sum(o["limited"] for o in orbit)) / max(1.0, float(sum(o["history_carrying_pixels"] for o in orbit)))}
    res["learning_passes"], res["replaces"] = h.info()["learning_passes"], h.info()["replaces"]
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

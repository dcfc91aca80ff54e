#!/usr/bin/env python3
"""What acn_denoise buys on scenes nobody asserted it on (reported, not asserted).

    python scripts/denoise_quality.py [--out profiles/r05/denoise_quality.json]

primitives_path and diamond_c4 of tests/scenes_util.SMALL: the frame at an eighth of the configuration's sampling, raw and
filtered with its FOLLOW records (defaults), and the frame at the configuration's own sampling, each against the frame at
sixteen times that sampling; MSE of clip( x, 0, 1 ), everything rendered on the device."""
import argparse
import json
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import actinon_amd as A
    import scenes_util as S

    mse = lambda x, ref: float(np.mean((np.clip(x, 0, 1) - np.clip(ref, 0, 1)) ** 2))
    res = {}
    for name in ("primitives_path", "diamond_c4"):
        builder, ov = S.SMALL[name]
        w, hh, p, d = ov["image_width"], ov["image_height"], ov["path_samples"], ov["direct_samples"]
        sc = A.Scene.build(builder, **ov)
        frames = {}
        for tag, (ps, ds) in (("eighth", (max(1, p // 8), max(1, d // 8))), ("own", (p, d)), ("reference", (16 * p, 16 * d))):
            sc.set(path_samples=ps, direct_samples=ds)
            flat = sc.flatten()
            pos = S.positions(flat)
            h = A.Handle(flat)
            frames[tag] = h.render_positions(pos, linear=True).reshape(hh, w, 3)
            if tag == "eighth":
                rec = h.surface_positions(pos, follow=True)
                frames["filtered"] = h.denoise(frames[tag], rec)
                hit = float(rec.hit.mean())
            h.close()
            frames[tag + "_samples"] = [ps, ds]
        e = {k: mse(frames[k], frames["reference"]) for k in ("eighth", "filtered", "own")}
        res[name] = {"size": [w, hh], "samples_eighth": frames["eighth_samples"], "samples_own": frames["own_samples"],
                     "samples_reference": frames["reference_samples"], "hit_fraction": hit,
                     "mse_raw_eighth": e["eighth"], "mse_filtered_eighth": e["filtered"], "mse_raw_own": e["own"],
                     "filtered_over_raw_eighth": e["filtered"] / e["eighth"], "filtered_over_raw_own": e["filtered"] / e["own"]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

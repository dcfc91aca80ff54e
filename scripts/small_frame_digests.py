"""sha256 of the linear radiance of the two small frames tests/test_gpu_frames_hard.py renders: the smoke workload of bench.py
(wine_glass 160 x 90, path 16 / direct 50) and the hanging_lamp fixture at 64 x 48 with its own sampling.
usage (on the GPU box): python scripts/small_frame_digests.py [OUT.json]     default: tests/golden/small_frame_digests.json
The committed digests are those of the build BEFORE a kernel change (scripts/regen_digests.sh runs this too): pixel sums are
order-independent fixed point, so a frame does not change with the kernels that add it up."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import actinon_amd as A   # noqa: E402
import bench              # noqa: E402

FRAMES = {
    "smoke": lambda: A.Scene.build(bench.WORKLOADS["smoke"][0], **bench.WORKLOADS["smoke"][1]).flatten(),
    "hanging_lamp_64x48": lambda: A.Flat.load(os.path.join(ROOT, "tests", "golden", "scenes", "hanging_lamp.npz"), image_width=64, image_height=48),
}


def digest(name):
    flat = FRAMES[name]()
    pos = A.main_pass_positions(int(flat.params.image_width), int(flat.params.image_height))
    h = A.Handle(flat)
    lin = h.render_positions(pos, linear=True)
    st = h.last_stages()
    h.close()
    return {"sha256": hashlib.sha256(lin.tobytes()).hexdigest(), "pixels": len(pos), "hard_rays": int(st["hard_rays"]), "probe_rays": int(st["probe_rays"])}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "small_frame_digests.json")
    res = {name: digest(name) for name in FRAMES}
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))

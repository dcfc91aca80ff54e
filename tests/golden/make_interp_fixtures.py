"""Generates tests/golden/interp/*.npz: what the interpreter (actinon_amd/host/acn_interp.c) makes of the reference's
shipped scripts that actinon_amd/host/acn_scenes.c also builds by direct API calls (primitives, wine_glass, diamond).

Run where a checkout of the reference is at hand, with the directory of its scripts as the argument:
    python tests/golden/make_interp_fixtures.py <reference checkout>/src_acn
A fixture is the OUTPUT of our interpreter on the script -- geometry, parameters and render-driver settings as numbers --
not the script.  Auto envelopes are skipped (A.Scene.AUTOENV_SKIP), as in tests/test_interp.py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import actinon_amd as A                      # noqa: E402

NAMES = ["primitives", "wine_glass", "diamond"]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    src = sys.argv[1]
    out_dir = os.path.join(HERE, "interp")
    os.makedirs(out_dir, exist_ok=True)
    for name in NAMES:
        sc = A.Scene.from_script(os.path.join(src, name + ".acn"), A.Scene.AUTOENV_SKIP)
        flat = sc.flatten()
        path = os.path.join(out_dir, name + ".npz")
        flat.save(path, driver=(sc.s.gradient_threshold, sc.s.gradient_samples, sc.s.gradient_cycles))
        print(f"{name}: {flat.n_nodes} nodes, {flat.c.n_elems} elems -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""The layers of the device code (actinon_amd/csrc/acn_device.h lists them; DESIGN.md section 4, "device headers") stay layers:
  - every layer header compiles as the only include of a unit, so it names what it needs itself;
  - the units that trace nothing -- denoise, the lens reductions, reprojection, select, the frame -- do not depend on a ray layer:
    a change to the leaves, the CSG machines, the prune programs, the traversals or the shading formulas cannot reach their code.
Compiles only (the compiler is $HIPCC, as in the Makefile); nothing runs on a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = "actinon_amd/csrc"

LAYERS = ["acn_dev_base.h", "acn_dev_scene.h", "acn_dev_image.h", "acn_dev_leaves.h", "acn_dev_machines.h", "acn_dev_prune.h",
          "acn_dev_traverse.h", "acn_dev_shading.h"]
RAY_LAYERS = ["acn_dev_leaves.h", "acn_dev_machines.h", "acn_dev_prune.h", "acn_dev_traverse.h", "acn_dev_shading.h",
              "acn_unimachine.h"]
RASTER_UNITS = ["k_denoise", "k_denoise_layers", "k_lens", "k_lens_surface", "k_lens_layers", "k_lens_layers_merge", "k_reproject",
                "k_select", "k_frame"]
# include paths and defines of the Makefile's HIPFLAGS (its defaults)
MAKE_FLAGS = ["-DACN_SHADE_WAVES=4", "-DACN_WALK_WAVES=4", "-DACN_TRACE_WAVES=4", "--offload-arch=gfx950", "-ffp-contract=off",
              "-fno-fast-math", "-Iinclude", "-I" + CSRC, "-std=c++17"]


def test_umbrella_is_the_layers_in_order():
    with open(os.path.join(ROOT, CSRC, "acn_device.h")) as f:
        inc = [ln.split('"')[1] for ln in f if ln.startswith("#include")]
    assert inc == LAYERS


@pytest.mark.parametrize("header", LAYERS)
def test_layer_header_is_self_contained(header, tmp_path):
    unit = tmp_path / "unit.hip"
    unit.write_text('#include "%s"\n' % header)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-x", "hip", "-std=c++17",
                        "-ffp-contract=off", "-Iinclude", "-I" + CSRC, str(unit)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("unit", RASTER_UNITS)
def test_raster_unit_sees_no_ray_layer(unit):
    r = subprocess.run([HIPCC] + MAKE_FLAGS + ["-MM", os.path.join(CSRC, unit + ".hip")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = {os.path.basename(w) for w in r.stdout.replace("\\\n", " ").split()}
    assert "acn_dev_base.h" in deps and "acn_dev_scene.h" in deps, deps   # (the listing is the real one)
    assert not deps & set(RAY_LAYERS), sorted(deps & set(RAY_LAYERS))

"""Whole frames through the two-phase hard-ray kernels against the digests of the build before them (tests/golden/
small_frame_digests.json, written by scripts/small_frame_digests.py on that build): the frame of bench.py's smoke workload and the
hanging_lamp fixture at 64 x 48.  Occlusion is an OR over the root's elements and pixel sums are order-independent fixed point, so
compacting the undecided rays must not move a bit of either frame."""
import hashlib
import json
import os
import sys

import pytest

import actinon_amd as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def digests():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import small_frame_digests as D
    with open(os.path.join(HERE, "golden", "small_frame_digests.json")) as f:
        return D, json.load(f)


@pytest.mark.parametrize("name", ["smoke", "hanging_lamp_64x48"])
def test_small_frame_equals_the_digest_of_the_build_before(digests, name):
    assert A.device_count() >= 1, "no HIP device: the gpu tests must run on the GPU box"
    D, golden = digests
    flat = D.FRAMES[name]()
    pos = A.main_pass_positions(int(flat.params.image_width), int(flat.params.image_height))
    h = A.Handle(flat)
    lin = h.render_positions(pos, linear=True)
    st = h.last_stages()
    h.close()
    assert len(pos) == golden[name]["pixels"]
    # both kinds of record met in the hard-shadow queue, as many as in the build before
    assert st["hard_rays"] == golden[name]["hard_rays"] > 0 and st["probe_rays"] == golden[name]["probe_rays"] > 0, st
    assert hashlib.sha256(lin.tobytes()).hexdigest() == golden[name]["sha256"]

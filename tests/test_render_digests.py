"""The bytes of the three overlay entries (dyb_render_meshes, dyb_render_meshes_var, dyb_render_scenes) against recorded SHA-256
digests - on the kernel emulator here, on cuda:0 under `-m gpu`.

tests/test_render_var.py and tests/test_render_scene.py compare the ragged and the scene entry with the uniform one; all three run
the same kernels, so that equality cannot see a change that moves all of them alike, and tests/test_render.py allows the picture
+-1 per channel.  tests/golden/g11_render_digests.json pins every output array (pictures; face_id, depth and vertex normals of the
uniform entry; mesh_id and face_id of the scene entry) of the small cases render_cases.DIGEST_CASES.  It was recorded by
tools/make_golden_render.py from the commit BEFORE the three entries were put on one kernel set, on the emulator and on an MI355X:
{"all": ...} where the two recordings agree, else one set under "emu" and one under "gfx950".  They did not: 32 of the 34 arrays
have the same digest on both, the depth map and the vertex normals of the synthetic-SMPL case differ (its vertices come from the
skinning kernel of the device under test, fp32 sums in its own order; its picture and face ids agree all the same) - so the file
holds both sets.  Nothing here has a tolerance."""
import json
import os

import pytest

from conftest import GOLDEN
from render_cases import DIGEST_CASES, dev, digests, emu_lib      # noqa: F401 (fixtures)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "g11_render_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(DIGEST_CASES))
def test_bytes_are_the_recorded_ones(dev, recorded, smpl_tabs, case):
    want = recorded.get("all") or recorded["emu" if dev == "cpu" else "gfx950"]
    got = digests(DIGEST_CASES[case](dev, smpl_tabs))
    assert sorted(got) == sorted(want[case]), case
    for name in sorted(got):
        assert got[name] == want[case][name], (case, name)

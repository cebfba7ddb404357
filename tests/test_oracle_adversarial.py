"""The C oracle (oracle/vrt_oracle.c) against the NumPy oracle (oracle/numpy_oracle.py) on the
adversarial volumes (tests/adversarial_volumes.py) at 8^3: material bytes up to 255, glass clutter,
filled faces, the solid, all-glass and empty volumes and the glass / grass lattice, from four cameras
inside the volume, colour-only and textured. The contract is tests/test_oracle_crosscheck.py's: hit
records and counters equal, colour within 1e-5 (only exp2 / log2 differ: glibc against NumPy)."""
import numpy as np
import pytest

import oracle
import voxelraytracer_amd as vrt
from adversarial_volumes import INSIDE, NAMES, base_params, camera, volumes
from harness import params_dict, synthetic_atlas
from oracle import numpy_oracle

N, W, H = 8, 20, 14


@pytest.mark.parametrize("textured", [False, True], ids=["colour", "textured"])
@pytest.mark.parametrize("cid", INSIDE)
@pytest.mark.parametrize("name", NAMES)
def test_c_oracle_matches_numpy_on_adversarial_volumes(built, name, cid, textured):
    vox = volumes(N)[name]
    cam = camera(N, cid, W, H)
    p = base_params()
    if textured:
        p = vrt.textured_params(p, synthetic_atlas(32, 16), 16)
    rgba_c, hits_c, cnt_c = oracle.render(cam, vox, N, p, threads=1)
    rgba_n, hits_n, cnt_n = numpy_oracle.render(list(cam.inv_pv), W, H, vox, N, params_dict(p))
    assert np.array_equal(hits_c["voxel_index"], hits_n["voxel_index"])
    assert np.array_equal(hits_c["ray_length"].view(np.uint32), hits_n["ray_length"].view(np.uint32))
    assert np.array_equal(hits_c["steps"], hits_n["steps"])
    assert np.array_equal(hits_c["flags"], hits_n["flags"])
    assert cnt_c == cnt_n
    d = float(np.abs(np.clip(rgba_c, 0, 1) - np.clip(rgba_n, 0, 1)).max())
    print(f"{name} {cid} {'textured' if textured else 'colour'}: max |colour difference| {d:.3e}")
    assert d <= 1e-5
    # the case is what its name says: no hit in the empty volume, no miss from inside a full one
    found = hits_c["voxel_index"] >= 0
    if name == "empty":
        assert not found.any() and cnt_c["secondary_rays"] == 0
    if name in ("solid", "glass_solid"):
        assert found.all()
    if name in ("glass_solid", "glass_clutter", "lattice"):
        assert cnt_c["secondary_rays"] > 0
    if textured and name != "empty":
        rgba_0, _, _ = oracle.render(cam, vox, N, base_params(), threads=1)
        assert np.abs(rgba_0 - rgba_c).max() > 1e-3   # the atlas is what colours it

"""GPU: the kernel's certified walks against the oracle's exact walks, ray by ray (vrt_debug_cert_walks), on the
directed ray lists of tests/cert_rays.py. A certified walk returns the exact walk's outcome or says "unsure":
every certain record of the device must be the exact walk's (air walk: found, byte, face axis, cell and the hit
parameter within the walk's own bound; shadow walk: the blocked bit), the certified pass's form of each walk
(its unguarded loads) must equal the guarded form word for word, "not started" must be reported exactly where
the start checks refuse the ray, and the device must not pass by answering "unsure": per class and kind its
certain share is at least half the CPU model's on the same rays (the kernel's factored float bound and the
model's double bound differ near the thresholds, which is what the factor allows for). The model
(scripts/certsim.c) is held to the same oracle by tests/test_cert_rays.py, with the conditions that keep the
lists from passing empty."""
import time

import numpy as np
import pytest

import cert_rays
import voxelraytracer_amd as vrt
from cert_rays import HIT, MISS, NOT_STARTED, describe, model_walks, parameter_error, unsound

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("vol", cert_rays.VOLUMES, ids=cert_rays.volume_id)
def test_device_walks_are_sound_on_directed_rays(built, vol):
    vname, n, dens = vol
    vox = cert_rays.volume(vname, n, dens)
    failures = []
    t_device = 0.0
    t0 = time.perf_counter()
    with vrt.Renderer(0) as r:
        r.set_skip_layout(8)   # the certified walks' skip field
        r.upload_volume(vox, n)
        for cls in cert_rays.CLASSES:
            rays = cert_rays.rays(vname, n, dens, cls)
            for kind in (0, 1):
                t1 = time.perf_counter()
                got = r.debug_cert_walks(rays, kind)
                lean = r.debug_cert_walks(rays, kind + 2)
                t_device += time.perf_counter() - t1
                exact = cert_rays.exact_walks(vox, n, rays, kind)
                model = model_walks(vox, n, rays, kind)
                what = (cert_rays.volume_id(vol), cls, kind)

                def fail(text, bad):
                    failures.append((what, text, int(np.count_nonzero(bad)), describe(rays, exact, got, bad)))

                # the record's words, lean against guarded
                differ = np.any(got.view(np.uint32).reshape(-1, 8) != lean.view(np.uint32).reshape(-1, 8), axis=1)
                if differ.any():
                    fail("the lean walk's record differs from the guarded walk's", differ)
                # not started: exactly where the start checks say
                refused = cert_rays.not_started(vox, n, rays, kind)
                if np.any((got["res"] == NOT_STARTED) != refused):
                    fail("'not started' differs from the start checks' restatement", (got["res"] == NOT_STARTED) != refused)
                assert np.all((got["res"] >= MISS) & (got["res"] <= NOT_STARTED)), what
                # soundness
                wrong = unsound(exact, got, kind)
                if wrong.any():
                    fail("certain outcomes that are not the exact walk's", wrong)
                if kind == 0:
                    hit = (got["res"] == HIT) & (exact["found"] != 0)
                    cell = got["cell"].astype(np.int64)
                    vidx = cell[:, 0] + n * (cell[:, 1] + n * cell[:, 2])
                    if np.any(hit & (vidx != exact["vidx"])):
                        fail("a certified hit's cell is not the exact walk's voxel", hit & (vidx != exact["vidx"]))
                    bound = got["eu"].astype(np.float64) + np.spacing(exact["len"]).astype(np.float64)
                    off = hit & ~(parameter_error(rays, exact, got) <= bound)
                    if off.any():
                        fail("|(len - len0) - u| > eu + ulp(len)", off)
                # not vacuous: the device's certain share against the model's
                dev_share = np.count_nonzero(got["res"] <= HIT) / len(rays)
                model_share = np.count_nonzero(model["res"] <= HIT) / len(rays)
                print(f"{what}: certain share device {dev_share:.4f}, model {model_share:.4f}; not started "
                      f"{np.count_nonzero(refused)}; unsound {np.count_nonzero(wrong)}")
                if not dev_share >= 0.5 * model_share:
                    failures.append((what, "the device's certain share is below half the model's", dev_share, model_share))
    print(f"{cert_rays.volume_id(vol)}: {time.perf_counter() - t0:.2f} s, of which the device's walks {t_device:.2f} s")
    assert not failures, (len(failures), failures[:6])

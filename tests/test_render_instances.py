"""The instance table of the frame kernels (csrc/vrt_instances.h, host arithmetic, no GPU): launch_render's
kernels are rows of two constexpr arrays and one function chooses a launch's rows. tests/render_instances_check.cpp,
a program of its own that includes only that header, is built here with the host sanitizers and run. Over
stats x textured x cert {0, 1, 2} x tree x order x defer x nframes {1, 2, 8} x exact_fat (six flags, 3 x 3 values: 576 launches) it holds
(a) the chosen rows equal to the two ternary cascades launch_render held before the table, restated in the program as
they were written; (b) exactly 22 render_kernel rows and 6 exact-pass rows, all distinct and each reached by some
launch; (c) the choice total: a row for every launch, an exact-pass row exactly for the deferred pairs.
The same program built with VRT_EXACT_VGPRS=0 (make variant builds without the VGPR cap) holds the uncapped pair."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "voxelraytracer_amd", "csrc")


def test_header_is_host_only():
    """vrt_instances.h includes <cstdint> and vrt_tuning.h, nothing else (nothing of HIP)."""
    with open(os.path.join(CSRC, "vrt_instances.h")) as f:
        incs = [l.split()[1] for l in f if l.startswith("#include")]
    assert incs == ["<cstdint>", '"vrt_tuning.h"'], incs


@pytest.mark.parametrize("defs,capped", [((), 2), (("-DVRT_DIAGNOSTIC_BUILD", "-DVRT_EXACT_VGPRS=0"), 0)])
def test_choice_equals_the_cascades(tmp_path, defs, capped):
    exe = str(tmp_path / "render_instances_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *defs, "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "render_instances_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    want = ("inputs 576 mismatches 0 render rows 22 distinct 22 reached 22 exact rows 6 distinct 6 reached 6 "
            "capped %d\nok\n" % capped)
    assert r.stdout == want, r.stdout

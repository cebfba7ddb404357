"""The pass list of a skip-field rebuild (csrc/vrt_skipfield_plan.cpp, host arithmetic, no GPU). fwd_pass_kernel and
dist_pass_kernel index their input box with no bounds test, on the promise "every read is inside ib"; the boxes
skipfield_passes gives them are what keeps it. tests/skipfield_passes_check.cpp, a program of its own, is built from
vrt_skipfield_plan.cpp alone with the host sanitizers and run. For octants in {8, 1} and distances in {0, 1} it
checks every pass of every box:
 (a) every region has extents >= 1, lies in [0, N)^3 and has at most N^3 cells;
 (b) a forward pass's output box lies inside its input box on the two other axes, and along the pass's axis so does
     the output box extended kFwdCap - 1 cells ahead in the pass's direction, clipped to the volume;
 (c) the same for a distance pass, with kDistCap - 1 cells to both sides;
 (d) a pass's input box is exactly the output box of the pass that wrote the scratch third it reads, and the whole
     volume for a first pass;
 (e) for the whole-volume box every region is the whole volume;
 (f) the packs' boxes equal vrt_volume_edit_plan's boxes (the edit's own box when the distances are kept);
and that the list is the rebuild's launches in their order (x -> y -> z nesting, a pack after each z pass, the edge
pack when the box holds coordinate 0 of an axis).
The boxes: at N = 2 and 4 every box of the volume, at N = 16 every box with extents in {1, 2, N}; at N = 256 and
1024, where the caps bind and the regions are regional, the whole volume, unit boxes at the 8 corners and the centre,
a box flush with each face and 2000 seeded random boxes. (b) to (d) hold for every one of them, not for a share."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "voxelraytracer_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("skipfield_passes") / "skipfield_passes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "skipfield_passes_check.cpp"),
                           os.path.join(CSRC, "vrt_skipfield_plan.cpp")])
    return exe


@pytest.mark.parametrize("n,boxes", [(2, 27), (4, 1000), (16, 32768), (256, 2016), (1024, 2016)])
def test_every_pass_reads_inside_its_input_box(checker, n, boxes):
    r = subprocess.run([checker, str(n)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert r.stdout == "ok n %d boxes %d\n" % (n, boxes), r.stdout


def test_plan_file_is_host_only():
    """vrt_skipfield_plan.{h,cpp} include nothing of HIP or RCCL (the build above links without either)."""
    for name in ("vrt_skipfield_plan.h", "vrt_skipfield_plan.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            incs = [l.split()[1] for l in f if l.startswith("#include")]
        assert all(i in ("<algorithm>", "<cstdint>", '"vrt_tuning.h"', '"vrt_skipfield_plan.h"') for i in incs), incs

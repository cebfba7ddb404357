"""The numeric A/B knobs of the kernels live in csrc/vrt_tuning.h behind one guard: a knob defined
without VRT_DIAGNOSTIC_BUILD (i.e. outside `make variant`) must stop the build, with a message that
names make variant builds; with VRT_DIAGNOSTIC_BUILD the same definition is accepted. The header
needs no HIP: it is preprocessed with the host C++ compiler."""
import os
import subprocess

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "voxelraytracer_amd", "csrc", "vrt_tuning.h")


def _preprocess(*defs):
    return subprocess.run(["g++", "-std=c++17", "-E", "-o", os.devnull, *defs, HDR],
                          capture_output=True, text=True)


def test_knob_needs_a_diagnostic_build():
    r = _preprocess("-DVRT_MIN_WAVES=6")
    assert r.returncode != 0
    assert "#error" in r.stderr and "make variant builds" in r.stderr


def test_knob_accepted_in_a_diagnostic_build():
    r = _preprocess("-DVRT_MIN_WAVES=6", "-DVRT_DIAGNOSTIC_BUILD")
    assert r.returncode == 0, r.stderr


def test_defaults_need_no_definition():
    r = _preprocess()
    assert r.returncode == 0, r.stderr

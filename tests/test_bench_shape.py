"""bench.py's pipeline decisions (no GPU): the compositor rule, frames per launch and lanes of a
K-way split, as the driver's N = 1/2/4/8 runs take them."""
import sys

import pytest

import bench


def shape(argv, world):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        args = bench.parse()
    finally:
        sys.argv = old
    return bench.compositor_on(args, world), bench.pipeline_shape(args, world)


@pytest.mark.parametrize("world,comp,batch", [(1, False, 1), (2, False, 2), (3, False, 3),
                                              (4, True, 3), (8, True, 8)])
def test_driver_defaults(world, comp, batch):
    c, (lanes, queues, b) = shape([], world)
    assert c is comp and b == batch and lanes == 4 and queues == 4


def test_flags():
    assert shape(["--no-gather"], 8)[0] is False                     # no gather, no compositor
    assert shape(["--compositor", "-1"], 8)[0] is False
    assert shape(["--compositor", "1"], 3)[0] is True
    assert shape(["--rehearse-ranks", "8", "--rehearse-gather"], 1)[0] is False
    c, (_, _, b) = shape(["--rehearse-ranks", "8", "--rehearse-gather", "--compositor", "1"], 1)
    assert c is True and b == 8                                      # the renderers' 7-way batches
    assert shape(["--alpha", "0.5"], 8)[1][2] == 1                   # dependent frames: no batches
    assert shape(["--batch", "3"], 8)[1][2] == 3


def test_checks_need_full():
    """--oracle-check / --verify-frames configure passes that only --full runs: asking for them
    without it is an error (before anything is initialised), never a silent no-check."""
    for argv in (["--oracle-check"], ["--verify-frames", "3"]):
        old = sys.argv
        sys.argv = ["bench.py"] + argv
        try:
            with pytest.raises(SystemExit) as e:
                bench.main()
        finally:
            sys.argv = old
        assert "--full" in str(e.value)


def test_dump_outputs(tmp_path):
    """--dump-outputs: a frame is written whole as float32; one above the size limit as the same
    sorted sample of its pixels every time, within the limit."""
    import numpy as np

    small = (np.arange(6 * 5 * 4) % 256).astype(np.uint8).reshape(6, 5, 4)
    bench.dump_outputs(str(tmp_path / "d"), "frame", small)
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.astype(np.float32))
    h, w = 2160, 3840   # C4's frame: 132.7 MB as float32
    big = (np.arange(h * w * 4, dtype=np.uint32) % 251).astype(np.uint8).reshape(h, w, 4)
    bench.dump_outputs(str(tmp_path / "a"), "frame", big)
    bench.dump_outputs(str(tmp_path / "b"), "frame", big)
    a, b = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 4
    assert a.nbytes <= bench.DUMP_LIMIT_BYTES < 64 * 10**6 and np.array_equal(a, b)
    # the sample's rows are whole pixels of the frame (channel c of pixel i is (4 i + c) % 251)
    assert a.shape[0] == bench.DUMP_LIMIT_BYTES // 16
    assert np.array_equal(a[:, 1:], (a[:, :1] + np.arange(1, 4)) % 251)

"""`upload.stage_rows`: the one place where host frames and masks are converted on their way into the staging buffers (numpy only)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rgbmanip_amd.upload import stage_rows

RANGES = ((0, 2), (2, 4), (4, 5))                # three chunks, the last one a single row


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=4) as p:
        yield p


def _stage_all(src, kind, dst_dtype, sentinel, pool):
    """Stage src chunk by chunk into the rows of one destination; after every chunk the rows outside [lo, hi) are what they were."""
    dst = np.full(src.shape, sentinel, dtype=dst_dtype)
    for lo, hi in RANGES:
        before = dst.copy()
        for f in stage_rows(dst[lo:], src, lo, hi, kind, pool, parts=3):
            f.result()
        assert np.array_equal(dst[:lo], before[:lo]) and np.array_equal(dst[hi:], before[hi:])
        assert (dst[hi:] == sentinel).all()
    return dst


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16, np.uint8])
def test_frames_are_cast_to_the_staging_dtype(dtype, pool):
    g = np.random.default_rng(3)
    if dtype == np.uint8:
        src = g.integers(0, 256, (5, 4, 6, 3), dtype=np.uint8)
        got = _stage_all(src, "frame", np.uint8, 7, pool)
        assert got.dtype == np.uint8 and np.array_equal(got, src)
    else:
        src = g.random((5, 4, 6, 3)).astype(dtype)
        got = _stage_all(src, "frame", np.float32, -3.0, pool)
        assert got.dtype == np.float32 and np.array_equal(got, src.astype(np.float32))


@pytest.mark.parametrize("dtype", [np.bool_, np.uint8, np.int64, np.float32, np.float64])
def test_masks_become_one_byte_per_pixel(dtype, pool):
    vals = np.array([0, 1, 255, -1, 0.5])
    with np.errstate(invalid="ignore"):
        src = np.resize(vals, 5 * 4 * 6).reshape(5, 4, 6).astype(dtype)      # (an integer type holds what the cast makes of them)
    assert (src == 0).any() and (src != 0).any()
    got = _stage_all(src, "mask", np.uint8, 9, pool)
    assert np.array_equal(got, (src != 0).astype(np.uint8))


def test_integer_frames_are_refused(pool):
    src = np.zeros((5, 4, 6, 3), dtype=np.int32)
    dst = np.zeros((5, 4, 6, 3), dtype=np.float32)
    with pytest.raises(TypeError, match=r"estimate: rgb frames must be float images in \[0, 1\] or uint8, got int32"):
        stage_rows(dst, src, 0, 2, "frame", pool)


def test_default_split_covers_the_rows_once(pool):
    src = np.arange(37 * 3, dtype=np.float64).reshape(37, 3)
    dst = np.zeros((37, 3), dtype=np.float32)
    futs = stage_rows(dst, src, 0, 37, "frame", pool)
    for f in futs:
        f.result()
    assert 1 <= len(futs) <= 37 and np.array_equal(dst, src.astype(np.float32))

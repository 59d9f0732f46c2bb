"""The detector stage from two host threads at once.  Its one-time device set-up (dynamic-LDS limits of the binning kernels,
the CIE observer table) is one record per device for the whole process (csrc/ot_detect_api.hip `detector_setup`), shared by every
thread.  Each thread traces its own seeded Raytracer and renders an image with a user extent (`ot_detector_images`) and
one with the one-pass automatic extent (`ot_detector_image_auto_*`); the results equal the same calls made in one thread."""
import threading

import numpy as np
import pytest

import optrace_amd as ot
import scenes

pytestmark = pytest.mark.gpu

N = 2_500_000  # above OT_TILE_MIN_HITS: the fused pass may take its tile path
EXTENT = [-4.5, 4.5, -3.5, 3.5]
SEEDS = (41, 42)


def images(seed):
    """-> (image with EXTENT, image with the automatic extent) of scene C4 traced with `seed`."""
    RT = scenes.c4_image_render(ot, seed=seed)
    one_pass = []
    orig = RT._auto_image_one_pass

    def spy(*a, **k):
        img = orig(*a, **k)
        one_pass.append(img is not None)
        return img

    RT._auto_image_one_pass = spy
    with ot.global_options.no_warnings():
        RT.trace(N)
        fused = RT.detector_image(extent=EXTENT)
        auto = RT.detector_image()
    assert one_pass == [True], "the automatic extent in one pass"
    return fused, auto


def same(a, b):
    A, B = a._data, b._data
    np.testing.assert_allclose(a.extent, b.extent, rtol=0, atol=1e-12)
    assert A.shape == B.shape
    assert A[..., 3].sum() > 0
    assert np.array_equal(A[..., 3] != 0, B[..., 3] != 0), "same pixels lit"
    np.testing.assert_allclose(A.sum(axis=(0, 1)), B.sum(axis=(0, 1)), rtol=1e-12, atol=0)


def test_detector_images_from_two_threads():
    old = ot.Raytracer.AUTO_ONE_PASS_FROM
    ot.Raytracer.AUTO_ONE_PASS_FROM = 1  # (set before the threads start)
    try:
        out, errors = {}, []
        start = threading.Barrier(len(SEEDS))

        def work(seed):
            try:
                start.wait()
                out[seed] = images(seed)
            except BaseException as e:  # (re-raised below, in the test's own thread)
                errors.append(e)

        threads = [threading.Thread(target=work, args=(s,)) for s in SEEDS]
        # (`no_warnings` is a process-wide switch: workers that leave it in another order than they entered it leave it off, and
        # the tests after this one would see no warning.  Leaving it here, after them, puts it back.)
        with ot.global_options.no_warnings():
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        if errors:
            raise errors[0]
        for seed in SEEDS:  # the same calls, one thread
            fused, auto = images(seed)
            same(out[seed][0], fused)
            same(out[seed][1], auto)
    finally:
        ot.Raytracer.AUTO_ONE_PASS_FROM = old

"""score_pull_form, the rule that chooses between the row scatter's two kernels: host code, no GPU."""
import pytest

from score_amd import _lib

GIB4 = 1 << 32


@pytest.mark.parametrize("D,want", [(16, 1), (32, 1), (64, 1), (4, 0), (8, 0), (12, 0), (20, 0), (48, 0), (60, 0), (128, 0),
                                    (256, 0), (0, 0), (-16, 0)])
def test_geometry(D, want):
    # a group of D/4 lanes has to fill whole DPP banks of one 16-lane row: 4, 8 or 16 lanes and no idle lane
    lib = _lib.load()
    assert lib.score_pull_form(D, 2, 1 << 20) == want
    assert lib.score_pull_form(D, 1, 1 << 20) == want


@pytest.mark.parametrize("mode,want", [(0, 0), (1, 1), (2, 1), (3, 0), (-1, 0)])
def test_mode(mode, want):
    # 0 is the owner-side row sum (score_segment_sum_rows): always pull_kernel
    lib = _lib.load()
    for D in (16, 32, 64):
        assert lib.score_pull_form(D, mode, 4096) == want


@pytest.mark.parametrize("span,want", [(1, 1), (GIB4 - 4, 1), (GIB4, 1), (GIB4 + 1, 0), (GIB4 + 4, 0), (1 << 40, 0), (0, 0),
                                       (-4, 0)])
def test_span_on_both_sides_of_4_gib(span, want):
    # every byte offset from the base has to fit 32 bits: the last byte of a span of exactly 4 GiB is 2^32 - 1
    lib = _lib.load()
    for D in (16, 32, 64):
        for mode in (1, 2):
            assert lib.score_pull_form(D, mode, span) == want


def test_no_launch_yet():
    assert _lib.load().score_pull_last_form() in (-1, 0, 1)

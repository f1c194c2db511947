"""CPU: the images of tests/_crf_rows.py really hold the contributor lists that test_crf_rows_gpu.py relies on.

The list lengths are read off the lattice keys of oracle/densecrf_ref.c::lattice_init as restated in _crf_rows.lattice_keys;
that restatement is held against the oracle itself: it must find exactly as many lattice points, on both lattices of every
image, as the oracle's own hash table does."""
import numpy as np
import pytest

import _crf_rows as CR
from oracle import pipeline_np as OP


@pytest.fixture(scope="module")
def lengths():
    return [(CR.list_lengths(rgb, 3.0), CR.list_lengths(rgb, 50.0, 5.0)) for rgb in CR.case(3).rgb]


def test_restated_lattice_has_the_oracles_point_counts(lengths):
    c = CR.case(3)
    for b, (lg, lb) in enumerate(lengths):
        h, w = c.sizes[b]
        _, _, stats = OP.densecrf(c.rgb[b], c.ref_blur(b, True), want_q=True, iters=0)
        assert [len(lg), len(lb)] == [int(stats[0]), int(stats[1])], (b, c.sizes[b])
        assert lg.sum() == 3 * h * w and lb.sum() == 6 * h * w


def test_every_image_holds_every_list_length(lengths):
    """1, G, G + 1, LPP and LPP + 1 entries for LPP = 8, 16, 32 on the bilateral lattice, lists beyond 2 * LPP on it (the flat
    background), and Gaussian lists past G and LPP = 8 / 16."""
    for b, (lg, lb) in enumerate(lengths):
        have = set(int(n) for n in lb)
        assert not [n for n in CR.WANT if n not in have], (b, sorted(have)[:40])
        assert lb.max() > 2 * max(CR.LPPS) + CR.G
        assert lg.max() > max(CR.G, 16) and 1 in set(int(n) for n in lg) | have


def test_sizes_are_small_and_odd_and_batches_have_a_tail_image():
    assert all(h <= 40 and w <= 64 and (h % 2 or w % 2) for h, w in CR.SIZES)
    assert len(CR.SIZES) == 9                                          # one round of 8 whole images + one sliced tail image
    for K in CR.KS:
        c = CR.case(K)
        assert c.K == [K] * 9 and all(np.array_equal(a, b) for a, b in zip(c.rgb, CR.case(3).rgb))


@pytest.mark.parametrize("K,single,paired", [(3, "8", "8"), (21, "8", "16"), (30, "8", "16"), (59, "16", "32"),
                                             (100, "32", "multi"), (151, "multi", "multi")])
def test_class_counts_cover_every_splat_dispatch(K, single, paired):
    """crf_filter's rule: chunks of the widest row <= 8 / 16 / 32 -> LPP 8 / 16 / 32, beyond -> MULTI."""
    def dispatch(kp):
        k4 = (kp + 3) // 4
        return "8" if k4 <= 8 else "16" if k4 <= 16 else "32" if k4 <= 32 else "multi"
    assert K in CR.KS
    assert dispatch((K + 3) // 4 * 4) == single and dispatch((2 * K + 3) // 4 * 4) == paired

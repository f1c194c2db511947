"""GPU: every dispatch of crf_splat_kernel on contributor lists of every length class (tests/_crf_rows.py: lists of 1, G,
G + 1, LPP, LPP + 1 and hundreds of entries in nine small odd-sized images with large flat-colour regions; what the images
hold is proven in test_crf_rows_cpu.py).  One batch of nine images per class count, single and paired, in one launch set
(one round of whole images per XCD + one tail image in eight slices): labels equal the oracle's, marginals to R.Q_ATOL, and
every image equals its own single-image run bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _crf_rows as CR                               # noqa: E402
import _post_refs as R                               # noqa: E402
from test_post_ops_gpu import _assert_oracle, _assert_runs_identical, _engine, _maxpix, _prepare, _run_single_and_pair, _total   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=CR.KS, ids=lambda K: f"K{K}")
def runs(request):
    case = CR.case(request.param)
    R.check_crf_input(case, True)
    R.check_crf_input(case, False, second=True)
    e = _engine(case.B, _total(case), _maxpix(case), max(case.K), 0, max_text_len=192)
    _prepare(e, case)
    batch = _run_single_and_pair(e, case)
    singles = []
    for b in range(case.B):
        sub = case.sub(b)
        _prepare(e, sub)
        singles.append(_run_single_and_pair(e, sub))
    e.close()
    return case, batch, singles


def test_batch_of_nine_equals_oracle(runs):
    case, batch, _ = runs
    _assert_oracle(case, batch, range(case.B))


def test_batch_of_nine_equals_single_image_runs(runs):
    case, batch, singles = runs
    for b in range(case.B):
        _assert_runs_identical(batch, singles[b], images=[b], other_images=[0])
    for key in ("hist", "h1", "hn"):
        np.testing.assert_array_equal(sum(s[key] for s in singles), batch[key])

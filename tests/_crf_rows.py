"""Cases of the contributor-list tests of the DenseCRF splat (test_crf_rows_cpu.py, test_crf_rows_gpu.py).

crf_splat_kernel walks the contributor list of a lattice point LPP records at a time (LPP = 8, 16 or 32 lanes per point, chosen
from the widest row of the batch; rows wider than 32 chunks take several passes: MULTI) and gathers G = 8 rows at a time, so
its paths are told apart by the LENGTH of a list: 1, G, G + 1, LPP, LPP + 1 and more than 2 * LPP entries (the continuation
loop over record chunks).  The images here are built to hold such lists on the bilateral lattice: a flat grey background (its
lattice points collect hundreds of pixels each) with short horizontal runs of saturated colours on it.  A run's colour is far
from every other colour of the image, so the six lattice points of its pixels belong to that run alone and their lists are
as long as the run is, or split in two where the run crosses a simplex boundary.  RUNS was chosen on the CPU so that every
length of WANT occurs in every image; test_crf_rows_cpu.py proves it on the lattice keys of oracle/densecrf_ref.c::lattice_init,
restated below in numpy (checked there against the oracle's own lattice sizes).

One batch per class count: the splat dispatch follows the widest row of a launch set, single (Kp = 4 * ceil(K / 4) floats)
and paired (two groups per row).

    K     single: Kp, dispatch        paired: Kp, dispatch
    3       4   LPP 8                   8   LPP 8
    21     24   LPP 8                  44   LPP 16
    30     32   LPP 8 (8 chunks: full) 60   LPP 16
    59     60   LPP 16                120   LPP 32
    100   100   LPP 32                200   MULTI (50 chunks: 2 passes)
    151   152   MULTI (38 chunks)     304   MULTI (76 chunks: 3 passes)

Nine images per batch: one full round of whole images per XCD and one tail image cut into eight slices (xcd_work)."""
import functools

import numpy as np

import _post_refs as R

F32 = np.float32
G, LPPS = 8, (8, 16, 32)
WANT = sorted({1, G, G + 1} | set(LPPS) | {l + 1 for l in LPPS})          # 1, 8, 9, 16, 17, 32, 33
KS = (3, 21, 30, 59, 100, 151)
SIZES = [(39, 63), (37, 61), (33, 45), (40, 63), (35, 57), (39, 47), (33, 63), (37, 51), (35, 45)]    # H <= 40, W <= 64, odd
GREY = (128, 128, 128)
COLOURS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (0, 0, 0), (255, 255, 255)]
# (row, first column, length, colour index): rows two apart, every colour on one row only
RUNS = [(1, 2, 1, 6), (3, 1, 8, 0), (5, 3, 9, 1), (7, 0, 16, 2), (9, 5, 17, 3), (11, 1, 32, 4), (13, 4, 33, 5), (15, 2, 40, 7)]


def flat_image(h, w):
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[:] = GREY
    for y, x0, n, c in RUNS:
        img[y, x0:x0 + n] = COLOURS[c]
    return img


@functools.lru_cache(maxsize=None)
def case(K):
    c = R.Case(SIZES, [K - 1] * len(SIZES), [True] * len(SIZES), seed=70 + K, n_class=max(21, K))
    c.rgb = [flat_image(h, w) for h, w in SIZES]
    return c


# ------------------------------------------------------------------------------------------ lattice keys
def lattice_keys(feature):
    """(N, d) float32 features -> (N, d + 1, d) int16 keys of the d + 1 simplex vertices of every point: the statements of
    oracle/densecrf_ref.c::lattice_init in float32, vectorised over the points."""
    f = np.ascontiguousarray(feature, dtype=F32)
    N, d = f.shape
    inv_std_dev = F32(np.sqrt(2.0 / 3.0) * (d + 1))
    scale = [F32(1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std_dev)) for i in range(d)]
    elevated = np.zeros((N, d + 1), dtype=F32)
    sm = np.zeros(N, dtype=F32)
    for j in range(d, 0, -1):
        cf = f[:, j - 1] * scale[j - 1]
        elevated[:, j] = sm - F32(j) * cf
        sm = sm + cf
    elevated[:, 0] = sm
    down, up_f = F32(1.0) / F32(d + 1), F32(d + 1)
    rem0 = np.zeros((N, d + 1), dtype=F32)
    total = np.zeros(N, dtype=np.int32)
    for i in range(d + 1):
        v = down * elevated[:, i]
        up, dn = np.ceil(v) * up_f, np.floor(v) * up_f
        rd2 = np.where(up - elevated[:, i] < elevated[:, i] - dn, up, dn).astype(np.int16).astype(np.int32)
        rem0[:, i] = rd2.astype(F32)
        total = (total.astype(F32) + rd2.astype(F32) * down).astype(np.int32)
    rank = np.zeros((N, d + 1), dtype=np.int32)
    diff = (elevated - rem0).astype(np.float64)
    for i in range(d):
        for j in range(i + 1, d + 1):
            lt = diff[:, i] < diff[:, j]
            rank[:, i] += lt
            rank[:, j] += ~lt
    rank += total[:, None]
    lo, hi = rank < 0, rank > d
    rank = rank + (d + 1) * lo - (d + 1) * hi
    rem0 = rem0 + F32(d + 1) * lo - F32(d + 1) * hi
    keys = np.empty((N, d + 1, d), dtype=np.int16)
    for rem in range(d + 1):
        canon = np.where(rank[:, :d] <= d - rem, rem, rem - (d + 1))
        keys[:, rem] = (rem0[:, :d] + canon.astype(F32)).astype(np.int16)
    return keys


def list_lengths(rgb, sxy, srgb=None):
    """Contributor-list length of every lattice point of an image: Gaussian lattice (srgb None) or bilateral."""
    h, w = rgb.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    cols = [xx.reshape(-1).astype(F32) / F32(sxy), yy.reshape(-1).astype(F32) / F32(sxy)]
    if srgb is not None:
        cols += [rgb[..., c].reshape(-1).astype(F32) / F32(srgb) for c in range(3)]
    keys = lattice_keys(np.stack(cols, axis=1))
    _, counts = np.unique(keys.reshape(-1, keys.shape[-1]), axis=0, return_counts=True)
    return counts

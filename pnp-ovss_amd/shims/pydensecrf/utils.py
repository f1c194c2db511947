"""pydensecrf.utils: unary_from_softmax on the host (numpy); the other helpers are not provided."""
import numpy as np


def unary_from_softmax(sm, scale=None, clip=1e-5):
    """Class probabilities (C, ...) -> unary energies (C, N) float32: -log(p), p mixed with the uniform distribution when
    `scale` is given (scale * p + (1 - scale) / C) and clipped to [clip, 1] unless clip is None."""
    sm = np.asarray(sm)
    n_cls = sm.shape[0]
    if scale is not None:
        if not 0 < scale <= 1:
            raise ValueError("scale must be in (0, 1]")
        sm = scale * sm + (1 - scale) * (np.ones(sm.shape) / n_cls)
    if clip is not None:
        sm = np.clip(sm, clip, 1.0)
    return -np.log(sm).reshape([n_cls, -1]).astype(np.float32)


def _missing(name):
    def fn(*a, **k):
        raise NotImplementedError(f"pydensecrf.utils.{name} is not provided by the pnp_ovss shim")
    fn.__name__ = name
    return fn


for _n in ("unary_from_labels", "compute_unary", "softmax_to_unary", "create_pairwise_gaussian", "create_pairwise_bilateral"):
    globals()[_n] = _missing(_n)
del _n

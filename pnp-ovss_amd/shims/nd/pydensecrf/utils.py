"""pydensecrf.utils of the N-D shim: the one utils module of pnp-ovss_amd/shims/pydensecrf (unary_from_softmax, ...) plus the two
feature builders addPairwiseEnergy is used with.

create_pairwise_gaussian / create_pairwise_bilateral follow pydensecrf's meshgrid(indexing='ij') code AS THIS PROJECT READS IT:
coordinate axes in the order of `shape` (for an (H, W) image: row / sdims[0] first, then column / sdims[1] -- not the x, y
order of DenseCRF2D.addPairwiseGaussian), every feature a float32 divided in place by its width, the image channels after the
coordinates.  Like the general shim's sign convention this is pinned by nothing the reference holds: check it against your
pydensecrf before relying on bit-level agreement with it.
"""
import importlib.util
import numbers
import os

import numpy as np

_path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "pydensecrf", "utils.py")
_spec = importlib.util.spec_from_file_location("_pnp_ovss_shim_utils", _path)
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)
globals().update({k: v for k, v in vars(_mod).items() if not k.startswith("_") and k not in ("create_pairwise_gaussian", "create_pairwise_bilateral")})
del _path, _spec, _mod


def _mesh(sdims, shape):
    if len(sdims) != len(shape):
        raise ValueError(f"sdims has {len(sdims)} values for {len(shape)} axes")
    mesh = np.array(np.meshgrid(*[range(int(s)) for s in shape], indexing="ij"), dtype=np.float32)
    for i, s in enumerate(sdims):
        mesh[i] /= np.float32(s)
    return mesh


def create_pairwise_gaussian(sdims, shape):
    """(len(shape), prod(shape)) float32: coordinate i of every point of the grid, divided by sdims[i]."""
    return _mesh(sdims, shape).reshape(len(shape), -1)


def create_pairwise_bilateral(sdims, schan, img, chdim=-1):
    """(len(sdims) + channels, points) float32: the coordinates as create_pairwise_gaussian gives them, then the channels of
    img divided by schan (a number, or one width per channel).  chdim: the channel axis of img, -1 = img has none."""
    img = np.asarray(img)
    feat = img[np.newaxis].astype(np.float32) if chdim == -1 else np.moveaxis(img, chdim, 0).astype(np.float32)
    if isinstance(schan, numbers.Number):
        feat /= np.float32(schan)
    else:
        if len(schan) != feat.shape[0]:
            raise ValueError(f"schan has {len(schan)} values for {feat.shape[0]} channels")
        for i, s in enumerate(schan):
            feat[i] /= np.float32(s)
    out = np.concatenate([_mesh(sdims, feat.shape[1:]), feat])
    return out.reshape(out.shape[0], -1)

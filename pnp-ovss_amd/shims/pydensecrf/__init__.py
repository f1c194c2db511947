"""Import shim: the part of pydensecrf's interface the reference's densecrf() uses (PnP_OVSS_0514_updated_segmentation.py:
1030-1074), served by pnp_ovss.crf on the GPU.  Opt in by putting this directory's parent (pnp-ovss_amd/shims) on sys.path;
pnp_ovss itself must be importable.  Anything outside the supported subset raises NotImplementedError: nothing is approximated.
"""
__pnp_ovss_shim__ = True

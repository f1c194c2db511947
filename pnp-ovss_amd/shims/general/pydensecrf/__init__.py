"""Import shim, general form: pnp-ovss_amd/shims/pydensecrf (the part of pydensecrf's interface the reference's densecrf() uses)
plus what pydensecrf users commonly do besides -- compat as a vector or matrix, one width per feature axis, the
startInference / stepInference / klDivergence loop, map -- served by pnp_ovss.crf on the GPU.  Opt in by putting this
directory's parent (pnp-ovss_amd/shims/general) on sys.path INSTEAD of pnp-ovss_amd/shims; pnp_ovss itself must be importable.
It is a package of its own, because the shim under pnp-ovss_amd/shims keeps refusing these calls: that one computes only what
is tied to the oracle, while the sign and symmetrisation of a vector / matrix compat and the KL formula here are this project's
reading of densecrf, pinned by nothing (see densecrf.py).  Anything outside the supported set raises NotImplementedError:
nothing is approximated.
"""
__pnp_ovss_shim__ = True
__pnp_ovss_shim_general__ = True

"""Import shim, N-D form: pydensecrf's interface for any number of pairwise terms over arbitrary features -- DenseCRF(N, K) with
addPairwiseEnergy, DenseCRF2D with any number of addPairwiseGaussian / addPairwiseBilateral, utils.create_pairwise_gaussian /
create_pairwise_bilateral -- served by pnp_ovss.crf.FeatureCRF on the GPU.  Opt in by putting this directory's parent
(pnp-ovss_amd/shims/nd) on sys.path INSTEAD of pnp-ovss_amd/shims or pnp-ovss_amd/shims/general; pnp_ovss itself must be
importable.  A package of its own, because both other shims keep refusing these calls.  A term has at most 6 features.
Anything outside the supported set raises NotImplementedError: nothing is approximated.
"""
__pnp_ovss_shim__ = True
__pnp_ovss_shim_nd__ = True

"""`BlipITM`, `compute_gradcam_ensemble` and `BlipOutputFeatures` (the return type of BlipITM.extract_features) under their
reference import path (Files to replace for BLIP/blip_image_text_matching.py:386, :183)."""
from pnp_ovss.model import BlipITM, BlipOutputFeatures, compute_gradcam_ensemble  # noqa: F401

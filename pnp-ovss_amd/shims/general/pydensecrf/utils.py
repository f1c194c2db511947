"""pydensecrf.utils of the general shim: the one utils module of pnp-ovss_amd/shims/pydensecrf, loaded from its file."""
import importlib.util
import os

_path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "pydensecrf", "utils.py")
_spec = importlib.util.spec_from_file_location("_pnp_ovss_shim_utils", _path)
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)
globals().update({k: v for k, v in vars(_mod).items() if not k.startswith("_")})
del _path, _spec, _mod

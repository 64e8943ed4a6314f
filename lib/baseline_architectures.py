from sm_hpss_mtl_amd.lib.baseline_architectures import *  # noqa: F401,F403

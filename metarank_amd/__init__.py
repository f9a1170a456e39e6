"""metarank_amd — MI355X-native /rank hot path for Metarank (feature assembly + LambdaMART scoring).

The product is libmrk_hip.so (metarank_amd/csrc, C ABI in include/mrk.h); this package is the
thin host-side mirror of the reference's interfaces used by tests and benchmarks.
"""
from ._native import MrkError, build, lib, reload_switches  # noqa: F401
from .booster import LIGHTGBM, XGBOOST, Context, HipBooster, default_context  # noqa: F401
from .index import HipIndex  # noqa: F401,E402
from .ranker import Batch, HipRanker, Server, debug_fused_lds  # noqa: F401,E402
from .request import Request, RequestSet  # noqa: F401,E402
from .trending import HipTrending, TrendingBuilder  # noqa: F401,E402
from .als import AlsBuilder  # noqa: F401,E402
from .eval import eval_scores, evaluate, labels_from_interactions  # noqa: F401,E402
from .train import Trainer, bin_bounds, fit_lambdamart, lambdarank_gradients  # noqa: F401,E402

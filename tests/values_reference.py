"""What mrk_values must return, from the existing oracle (no oracle change).

ItemValue.fromState (model/ItemValue.scala:32-69) emits, per item, the values of the mapping's RankingFeatures (local_time, ua,
referer) in `features:` order followed by those of its ItemFeatures in `features:` order.  A model that lists the features in
that order has exactly those columns in its online matrix - which the oracle assembles -, and ValueMode.OfflineTraining differs
from it in the `position` columns only (PositionFeature.scala:32-33: the item's index in the request instead of the
configured constant; `grep OfflineTraining` over the reference finds no other reader).
"""
from __future__ import annotations

import copy

import numpy as np

RANKING_FEATURE_TYPES = ("local_time", "ua", "referer")   # the classes that extend RankingFeature
EMISSION_MODEL = "values_in_emission_order"


def emission_order(features) -> list:
    ranking = [f["name"] for f in features if f["type"] in RANKING_FEATURE_TYPES]
    item = [f["name"] for f in features if f["type"] not in RANKING_FEATURE_TYPES]
    return ranking + item


def with_emission_model(config: dict) -> dict:
    """the config plus a lambdamart model whose features are the whole mapping in emission order"""
    cfg = copy.deepcopy(config)
    cfg.setdefault("models", {})[EMISSION_MODEL] = {"type": "lambdamart", "features": emission_order(cfg["features"])}
    return cfg


def to_offline(matrix: np.ndarray, offsets: dict, features) -> np.ndarray:
    """the online matrix of ONE request -> its offline form; offsets: {feature name: (first column, dim)} of the matrix"""
    out = matrix.copy()
    for f in features:
        if f["type"] == "position" and f["name"] in offsets:
            out[:, offsets[f["name"]][0]] = np.arange(len(out), dtype=np.float64)
    return out


class ValuesOracle:
    """the oracle behind the emission-order model (or behind a named model of the config): expected(event, offline)"""

    def __init__(self, config: dict, model: str | None = None):
        from backends import OracleBackend

        self.config = with_emission_model(config)
        self.backend = OracleBackend(self.config, model or EMISSION_MODEL)
        self.offsets = self.backend.plan.offsets
        self.dim = self.backend.dim

    def expected(self, event: dict, offline: bool = True) -> np.ndarray:
        m = self.backend.matrix(event)
        return to_offline(m, self.offsets, self.config["features"]) if offline else m


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """bit for bit, NaN patterns included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))

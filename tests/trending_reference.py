"""Scalar Python restatement of the trending recommender's semantics the device fit reproduces (include/mrk.h,
mrk_trending_*): TrendingPredictor.fit / loadSync and TrendingModel.predict / save, ml/recommend/TrendingRecommender.scala,
with model/Timestamp.scala:11-24 and util/DurationJson.scala:9-13.  One interaction and one f64 operation at a time (Python
floats are IEEE doubles and fuse nothing); math.pow is the libm the library's host half calls."""
import math
import struct

import numpy as np

DAY_MS = 86_400_000
CANONICAL_NAN = np.uint64(0x7FF8000000000000)
OK, ERR_INVALID_ARG, ERR_PARSE, ERR_DIM_MISMATCH, ERR_UNSUPPORTED, ERR_NOT_FOUND = 0, -1, -2, -4, -6, -7


class Refused(Exception):
    def __init__(self, status, message):
        super().__init__(f"[{status}] {message}")
        self.status = status


def bits(x) -> np.ndarray:
    """bit patterns of doubles, NaNs canonicalised as java.lang.Double.doubleToLongBits does (knn_reference.bits)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = CANONICAL_NAN
    return b


def duration_ms(text: str) -> int:
    """DurationJson.scala:9-13: ([0-9]+)([smhd])"""
    unit = {"s": 1000, "m": 60_000, "h": 3_600_000, "d": DAY_MS}
    if len(text) < 2 or not text[:-1].isascii() or not text[:-1].isdigit() or text[-1] not in unit:
        raise Refused(ERR_PARSE, "duration is in wrong format: " + text)
    return int(text[:-1]) * unit[text[-1]]


def weights_of(config: dict) -> list:
    """InteractionWeight's decoder, :137-152: (interaction, weight, decay, window_ms, days) with the defaults 1.0, 1.0, 30d"""
    out = []
    for w in config["weights"]:
        window = duration_ms(w["window"]) if w.get("window") is not None else 30 * DAY_MS
        weight = 1.0 if w.get("weight") is None else float(w["weight"])
        decay = 1.0 if w.get("decay") is None else float(w["decay"])
        if any(o[0] == w["interaction"] for o in out):
            raise Refused(ERR_UNSUPPORTED, "two weights name the interaction " + w["interaction"])   # (rule 10: refused, not the .toMap)
        out.append((w["interaction"], weight, decay, window, window // DAY_MS))
    return out


def _java_key(score: float) -> int:
    """an unsigned key whose order is java.lang.Double.compare's order of -score (sortBy(-_.score), :85)"""
    neg = -score
    b = 0x7FF8000000000000 if neg != neg else struct.unpack("<Q", struct.pack("<d", neg))[0]
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def _pow(decay: float, i: int) -> float:
    try:
        return math.pow(decay, float(i))
    except OverflowError:         # libm returns the infinity (of the sign the odd / even exponent gives)
        return math.copysign(math.inf, -1.0 if decay < 0 and i % 2 else 1.0)


def _mul(a: float, b: float) -> float:
    return float(np.float64(a) * np.float64(b))     # (np.float64: inf * 0 is NaN without an exception, as IEEE says)


def fit(config: dict, ids, types, ts):
    """TrendingPredictor.fit, :39-87: (ids, scores) in model order"""
    weights = weights_of(config)
    n = len(ids)
    if n == 0:
        raise Refused(ERR_NOT_FOUND, "no interactions found")                        # :45
    now = max(int(t) for t in ts)                                                    # :45: every interaction, whatever its type
    items = list(dict.fromkeys(ids))                                                 # :47: distinct, first appearance
    grouped = []
    for name, _weight, _decay, window_ms, days in weights:                           # :50-65
        counts = {}
        for k in range(n):
            if int(ts[k]) > now - window_ms and types[k] == name:                    # :52-53, isAfter is strict
                day = (now - int(ts[k])) // DAY_MS                                   # :57
                arr = counts.setdefault(ids[k], [0] * days)
                if day >= days:                                                      # :58-59: ArrayIndexOutOfBounds
                    raise Refused(ERR_DIM_MISMATCH, f"weight {name}: day bucket {day} of {days}")
                arr[day] += 1
        grouped.append(counts)
    scores = []
    with np.errstate(all="ignore"):
        for item in items:                                                           # :66-83
            parts = []
            for (name, weight, decay, _w, days), counts in zip(weights, grouped):
                arr = counts.get(item)
                if arr is None:
                    parts.append(0.0)                                                # :79
                    continue
                s = 0.0
                for i in range(days):                                                # :72-77: every day, zero counts included
                    s = s + _mul(float(arr[i]), _pow(decay, i))
                parts.append(_mul(s, weight))                                        # :78
            total = 0.0
            for k, p in enumerate(parts):                                            # :82: List.sum as a reduce from the first part
                total = p if k == 0 else total + p
            scores.append(total)
    order = sorted(range(len(items)), key=lambda k: (_java_key(scores[k]), k))       # :85: stable sortBy(-score)
    return [items[k] for k in order], np.array([scores[k] for k in order], dtype=np.float64)


def save(ids, scores) -> bytes:
    """TrendingModel.save, :123-133 (ids as UTF-8 bytes: equal to writeUTF's for everything in the BMP except U+0000)"""
    out = [struct.pack(">ii", 1, len(ids))]
    for i, s in zip(ids, scores):
        raw = i.encode("utf-8", "surrogatepass") if isinstance(i, str) else i
        if len(raw) > 65535:
            raise Refused(ERR_UNSUPPORTED, "writeUTF: encoded string too long")
        out.append(struct.pack(">H", len(raw)) + raw + struct.pack(">d", s))
    return b"".join(out)


def predict(ids, scores, count: int):
    """TrendingModel.predict, :116-121"""
    if count <= 0:
        raise Refused(ERR_INVALID_ARG, "count should be greater than 0")
    return ids[:count], scores[:count]


def fit_numpy(config: dict, item_idx, type_idx, type_names, ts, n_items: int):
    """the same fit over integer-coded arrays in numpy (np.add.at counts + the same ordered sum): the CPU side of
    tools/trending_bench.py.  item_idx must number the items in order of first appearance.  Returns (order, scores by item)."""
    weights = weights_of(config)
    ts = np.asarray(ts, dtype=np.int64)
    now = int(ts.max())
    score = None
    with np.errstate(all="ignore"):
        for name, weight, decay, window_ms, days in weights:
            sel = (ts > now - window_ms) & (np.asarray(type_idx) == type_names.index(name)) if name in type_names else np.zeros(len(ts), bool)
            day = (now - ts[sel]) // DAY_MS
            if len(day) and int(day.max()) >= days:
                raise Refused(ERR_DIM_MISMATCH, f"weight {name}")
            table = np.zeros((days, n_items), dtype=np.uint32)
            np.add.at(table, (day, np.asarray(item_idx)[sel]), 1)
            s = np.zeros(n_items)
            for i in range(days):
                s = s + table[i].astype(np.float64) * _pow(decay, i)
            part = np.where(table.any(axis=0), s * weight, 0.0)
            score = part if score is None else score + part
    if score is None:
        score = np.zeros(n_items)
    neg = -score
    b = bits(neg)
    key = np.where((b >> np.uint64(63)).astype(bool), ~b, b | np.uint64(1 << 63))
    return np.lexsort((np.arange(n_items), key)), score


# TrendingRecommenderTest.scala:18-72: the config and the three known answers as (ids, types, ts, expected model)
TEST_CONFIG = {"weights": [{"interaction": "purchase", "weight": 5.0, "decay": 0.5}, {"interaction": "click", "weight": 1.0, "decay": 0.5}]}
_NOW = 1_700_000_000_000
KNOWN_ANSWERS = {
    "count clicks for today": (["p1", "p2", "p3", "p2", "p2"], ["click"] * 5, [_NOW] * 5, [("p2", 3.0), ("p1", 1.0), ("p3", 1.0)]),
    "decay for prev days": (["p1", "p2", "p3", "p2"], ["click"] * 4, [_NOW, _NOW, _NOW, _NOW - DAY_MS], [("p2", 1.5), ("p1", 1.0), ("p3", 1.0)]),
    "combine by weight": (["p1", "p2", "p3", "p2"], ["click", "click", "click", "purchase"], [_NOW] * 4, [("p2", 6.0), ("p1", 1.0), ("p3", 1.0)]),
}

"""numpy restatement of the similar-items semantics the device index reproduces (include/mrk.h, mrk_index_*): hnswlib-core's
DOUBLE_COSINE_DISTANCE, HnswIndexReader.lookup / centroid (ml/recommend/embedding/HnswJavaIndex.scala:23-59),
EmbeddingSimilarityModel.predict (ml/recommend/MFRecommender.scala:66-80) and Recommender.recommend's ordering
(ml/Recommender.scala:42).

Every sum walks the dimensions in order with one elementwise multiply and one elementwise add per step (numpy fuses
nothing), so a (query, row) pair sees exactly the spec's sequence of f64 operations."""
import numpy as np

CANONICAL_NAN = np.uint64(0x7FF8000000000000)


def bits(x) -> np.ndarray:
    """bit patterns of doubles, NaNs canonicalised as java.lang.Double.doubleToLongBits does"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = CANONICAL_NAN
    return b


def asc_key(x) -> np.ndarray:
    """unsigned keys whose integer order is java.lang.Double.compare's order (-0.0 < 0.0, NaN last)"""
    b = bits(x)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def distances(table, u) -> np.ndarray:
    v = np.asarray(table, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    rows, dim = v.shape
    dot = np.zeros(rows)
    nrv = np.zeros(rows)
    nru = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(dim):
            dot = dot + u[i] * v[:, i]
            nru = nru + u[i] * u[i]
            nrv = nrv + v[:, i] * v[:, i]
        return 1.0 - dot / (np.sqrt(nru) * np.sqrt(nrv))


def search(table, u, n):
    """the n nearest rows (all when the table has fewer), ascending by (Double.compare(distance), row)"""
    d = distances(table, u)
    order = np.lexsort((np.arange(len(d)), asc_key(d)))[: max(n, 0)]
    return order.astype(np.int32), d[order]


def centroid(vectors) -> np.ndarray:
    total = np.zeros(len(vectors[0]))
    with np.errstate(all="ignore"):
        for v in vectors:          # request order, sequential per dimension
            total = total + np.asarray(v, dtype=np.float64)
        return total / len(vectors)


def lookup(ids, table, items, n):
    """KnnIndexReader.lookup(items, n)"""
    table = np.asarray(table, dtype=np.float64)
    row_of = {s: i for i, s in enumerate(ids)}
    known = [row_of[s] for s in items if s in row_of]
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0))
    if not items or not known:
        return empty      # (several items, none known: a NaN centroid in the reference - undefined there, nothing here)
    query = table[known[0]] if len(items) == 1 else centroid([table[r] for r in known])
    return search(table, query, n)


def recommend_order(rows, score, request_rows, count):
    """filterNot(request.items.contains) + take(count) + stable sortBy(-score) under Double.compare"""
    keep = [i for i in range(len(rows)) if int(rows[i]) not in set(int(r) for r in request_rows)][: max(count, 0)]
    rows = np.asarray(rows)[keep]
    score = np.asarray(score, dtype=np.float64)[keep]
    order = np.argsort(asc_key(-score), kind="stable")
    return rows[order].astype(np.int32), score[order]


def recommend(ids, table, items, count):
    if not items:
        raise ValueError("similar items recommender requires request.items to be non-empty")
    rows, dist = lookup(ids, table, items, count + len(items))
    row_of = {s: i for i, s in enumerate(ids)}
    r, s = recommend_order(rows, dist, [row_of[i] for i in items if i in row_of], count)
    if len(r) == 0:
        raise LookupError("empty response from the recommender")
    return r, s

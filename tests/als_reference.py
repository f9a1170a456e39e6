"""Python restatement of the similar-items fit the device reproduces (include/mrk.h, mrk_als_*): the input
rules of MFPredictor.uirt (ml/recommend/MFRecommender.scala:44-63), ALSConfig's decoder and the fixed settings of ALSRecImpl.train
(ml/recommend/mf/ALSRecImpl.scala:18-81), and element-wise ALS as in He, Zhang, Kan, Chua, "Fast Matrix Factorization for Online
Recommendation with Implicit Feedback" (SIGIR 2016), Algorithm 1 / Eq. 12-13.  librec, which the reference runs, is not restated:
this is the library's stated definition.

Two forms.  `fit_loop` walks one row, one factor and one f64 operation at a time (Python floats are IEEE doubles and fuse
nothing) and is the bit reference.  `fit_numpy` does the same operations for all rows at once - numpy's element-wise + - * / are
the same IEEE operations - in the same order of summation, and must agree with the loop form to the bit.

Order of summation (a function of each sum's length alone):
  wave sum  - the L terms of a row's sum (over its entries; over k = 0 .. K-1): 64 partials, partial l = the terms l, l + 64, ...
              added in that order to +0.0; then for s = 32, 16, 8, 4, 2, 1: partial[l] = partial[l] + partial[l + s] for l < s;
              the sum is partial[0].  The excluded term k = f of the k-sum is +0.0.
  dot       - r_ui = p_u . q_i: k = 0 .. K-1 in order, added to +0.0.
  product   - S[f][k]: rows in chunks of 512 consecutive rows; a chunk's terms added in row order to +0.0; the chunk sums added in
              chunk order to +0.0.
"""
import math
import struct

import numpy as np

W0 = 128.0          # rec.eals.overall, ALSRecImpl.scala:27
ALPHA = 0.4         # rec.eals.ratio, :28
INIT_STD = 0.01
GRAM_CHUNK = 512
MAX_FACTORS = 256
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).copy()


def f32(x: float) -> float:
    """(double)(float)x: a Java float in f64 arithmetic"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def parse_config(config: dict) -> dict:
    """ALSConfig's decoder, ALSRecImpl.scala:60-81: the item regulariser comes from the key `itemRef` (:66); `itemReg` is ignored"""
    def opt(key, default):
        return default if config.get(key) is None else config[key]
    return {"iterations": int(opt("iterations", 100)), "factors": int(opt("factors", 100)),
            "lambda_user": f32(float(opt("userReg", 0.01))), "lambda_item": f32(float(opt("itemRef", 0.01)))}


class Problem:
    """users / items interned in order of first appearance, duplicate pairs collapsed, R_u ascending by item, R_i ascending by user,
    c_i = (w0 * p_i^alpha) / Z with p_i = n_i / nnz and Z summed in item order (math.pow is the libm the library's host half calls)"""

    def __init__(self, user_ids, item_ids):
        self.users, self.items = [], []
        uo, io = {}, {}
        pairs = set()
        for u, i in zip(user_ids, item_ids):
            if u not in uo:
                uo[u] = len(self.users)
                self.users.append(u)
            if i not in io:
                io[i] = len(self.items)
                self.items.append(i)
            pairs.add((uo[u], io[i]))
        self.pairs = len(user_ids)
        self.nnz = len(pairs)
        self.user_rows = [[] for _ in self.users]
        self.item_rows = [[] for _ in self.items]
        for u, i in sorted(pairs):
            self.user_rows[u].append(i)
            self.item_rows[i].append(u)
        pw = [math.pow(len(r) / self.nnz, ALPHA) for r in self.item_rows]
        z = 0.0
        for v in pw:
            z = z + v
        self.conf = [W0 * v / z for v in pw]

    def csr(self, rows):
        off = np.zeros(len(rows) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(r) for r in rows])
        return off, np.array([e for r in rows for e in r], dtype=np.int32)


# ---- the generator of the initial factors (csrc/als_host.hpp)

def _mix(x: int) -> int:
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ x >> 31


def init_value(seed: int, matrix: int, row: int, col: int) -> float:
    h = _mix(_mix(_mix(seed + GOLDEN * (matrix + 1) & M64) + row & M64) + col & M64)
    a, b = _mix(h + GOLDEN & M64), _mix(h + 2 * GOLDEN & M64)
    u1, u2 = float((a >> 11) + 1) * 2.0 ** -53, float(b >> 11) * 2.0 ** -53
    radius = math.sqrt(-2.0 * math.log(u1))
    return INIT_STD * (radius * math.cos(6.283185307179586 * u2))


def init_matrix(seed: int, matrix: int, rows: int, cols: int) -> np.ndarray:
    return np.array([[init_value(seed, matrix, r, c) for c in range(cols)] for r in range(rows)], dtype=np.float64).reshape(rows, cols)


# ---- the loop form

def wave_sum(terms) -> float:
    part = [0.0] * 64
    for j, t in enumerate(terms):
        part[j & 63] = part[j & 63] + t
    s = 32
    while s >= 1:
        for l in range(s):
            part[l] = part[l] + part[l + s]
        s >>= 1
    return part[0]


def gram_loop(M, weights):
    """S[f][k] = sum over rows r of (weights[r] *) (M[r][f] * M[r][k]); weights None: unweighted"""
    K = len(M[0])
    chunks = []
    for r0 in range(0, len(M), GRAM_CHUNK):
        acc = [[0.0] * K for _ in range(K)]
        for r in range(r0, min(len(M), r0 + GRAM_CHUNK)):
            row = M[r]
            for f in range(K):
                a, mf = acc[f], row[f]
                if weights is None:
                    for k in range(K):
                        a[k] = a[k] + mf * row[k]
                else:
                    c = weights[r]
                    for k in range(K):
                        a[k] = a[k] + c * (mf * row[k])
        chunks.append(acc)
    S = [[0.0] * K for _ in range(K)]
    for acc in chunks:
        for f in range(K):
            for k in range(K):
                S[f][k] = S[f][k] + acc[f][k]
    return S


def sweep_loop(rows, own, other, S, conf, lam, item_side):
    """re-solves every row of `own` in place.  rows[x] = the entries of row x (indices into `other`); conf = c_i per ITEM"""
    K = len(S)
    for x, entries in enumerate(rows):
        p = own[x]
        r = []
        for e in entries:
            q, acc = other[e], 0.0
            for k in range(K):
                acc = acc + p[k] * q[k]
            r.append(acc)
        wc = [1.0 - (conf[x] if item_side else conf[e]) for e in entries]   # w - c_i, w = 1
        for f in range(K):
            pf, Sf = p[f], S[f]
            qf = [other[e][f] for e in entries]
            rf = [r[j] - pf * qf[j] for j in range(len(entries))]
            num = wave_sum((1.0 - wc[j] * rf[j]) * qf[j] for j in range(len(entries)))   # w * r = 1
            den = wave_sum(wc[j] * (qf[j] * qf[j]) for j in range(len(entries)))
            ks = wave_sum(0.0 if k == f else p[k] * Sf[k] for k in range(K))
            if item_side:
                c = conf[x]
                new = (num - c * ks) / ((den + c * Sf[f]) + lam)
            else:
                new = (num - ks) / ((den + Sf[f]) + lam)
            r = [rf[j] + new * qf[j] for j in range(len(entries))]
            p[f] = new


def fit_loop(cfg: dict, pr: Problem, P0, Q0, iterations=None, each=None):
    """(P, Q) after cfg["iterations"] iterations from the initial matrices; `each(P, Q)` is called after every iteration"""
    P = [[float(v) for v in row] for row in np.asarray(P0, dtype=np.float64)]
    Q = [[float(v) for v in row] for row in np.asarray(Q0, dtype=np.float64)]
    for _ in range(cfg["iterations"] if iterations is None else iterations):
        Sq = gram_loop(Q, pr.conf)
        sweep_loop(pr.user_rows, P, Q, Sq, pr.conf, cfg["lambda_user"], False)
        Sp = gram_loop(P, None)
        sweep_loop(pr.item_rows, Q, P, Sp, pr.conf, cfg["lambda_item"], True)
        if each:
            each(np.array(P), np.array(Q))
    return np.array(P, dtype=np.float64).reshape(len(P), -1), np.array(Q, dtype=np.float64).reshape(len(Q), -1)


# ---- the numpy form

def _fold(part):
    s = 32
    while s >= 1:
        part = part[:, :s] + part[:, s:2 * s]
        s >>= 1
    return part[:, 0]


class _Rows:
    """the entries of all rows flattened, with the (row, partial, round) of each: round t holds every row's entries 64 t .. 64 t + 63"""

    def __init__(self, rows):
        self.n = len(rows)
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.row = np.repeat(np.arange(self.n), lens)
        self.idx = np.array([e for r in rows for e in r], dtype=np.int64)
        start = np.repeat(np.cumsum(lens) - lens, lens)
        j = np.arange(len(self.idx)) - start
        self.slot = j & 63
        rnd = j >> 6
        self.rounds = [np.nonzero(rnd == t)[0] for t in range(int(rnd.max()) + 1 if len(rnd) else 0)]

    def wave_sum(self, terms):
        part = np.zeros((self.n, 64))
        for sel in self.rounds:
            at = (self.row[sel], self.slot[sel])
            part[at] = part[at] + terms[sel]
        return _fold(part)


def _wave_sum_dense(T):
    """the wave sum of every row of T (rows x L): absent terms are +0.0, which leaves a partial's bits (a partial is never -0.0)"""
    n, L = T.shape
    pad = np.zeros((n, (L + 63) // 64 * 64))
    pad[:, :L] = T
    part = np.zeros((n, 64))
    for t in range(0, pad.shape[1], 64):
        part = part + pad[:, t:t + 64]
    return _fold(part)


def gram_numpy(M, weights):
    n, K = M.shape
    chunks = (n + GRAM_CHUNK - 1) // GRAM_CHUNK
    acc = np.zeros((chunks, K, K))
    for t in range(min(GRAM_CHUNK, n)):
        r = np.arange(t, n, GRAM_CHUNK)
        prod = M[r][:, :, None] * M[r][:, None, :]
        if weights is not None:
            prod = weights[r][:, None, None] * prod
        acc[:len(r)] = acc[:len(r)] + prod
    S = np.zeros((K, K))
    for c in range(chunks):
        S = S + acc[c]
    return S


def sweep_numpy(R: _Rows, own, other, S, conf, lam, item_side):
    K = S.shape[0]
    r = np.zeros(len(R.idx))
    for k in range(K):
        r = r + own[R.row, k] * other[R.idx, k]
    wc = 1.0 - (conf[R.row] if item_side else conf[R.idx])
    for f in range(K):
        qf = other[R.idx, f]
        rf = r - own[R.row, f] * qf
        num = R.wave_sum((1.0 - wc * rf) * qf)
        den = R.wave_sum(wc * (qf * qf))
        T = own * S[f][None, :]
        T[:, f] = 0.0
        ks = _wave_sum_dense(T)
        if item_side:
            new = (num - conf * ks) / ((den + conf * S[f, f]) + lam)
        else:
            new = (num - ks) / ((den + S[f, f]) + lam)
        r = rf + new[R.row] * qf
        own[:, f] = new


def fit_numpy(cfg: dict, pr: Problem, P0, Q0, iterations=None):
    P, Q = np.array(P0, dtype=np.float64), np.array(Q0, dtype=np.float64)
    conf = np.array(pr.conf, dtype=np.float64)
    Ru, Ri = _Rows(pr.user_rows), _Rows(pr.item_rows)
    for _ in range(cfg["iterations"] if iterations is None else iterations):
        sweep_numpy(Ru, P, Q, gram_numpy(Q, conf), conf, cfg["lambda_user"], False)
        sweep_numpy(Ri, Q, P, gram_numpy(P, None), conf, cfg["lambda_item"], True)
    return P, Q


# ---- checks of the restatement itself

def loss(cfg: dict, pr: Problem, P, Q) -> float:
    """the eALS objective (the paper's Eq. 8 with the reference's weights): sum over the entries of w (r - r^)^2, over the missing
    cells of c_i r^^2, plus lambda_u |P|^2 + lambda_i |Q|^2"""
    pred = P @ Q.T
    seen = np.zeros(pred.shape, dtype=bool)
    for u, row in enumerate(pr.user_rows):
        seen[u, row] = True
    c = np.array(pr.conf)[None, :]
    return float(((1.0 - pred) ** 2)[seen].sum() + (np.broadcast_to(c, pred.shape) * pred ** 2)[~seen].sum() +
                 cfg["lambda_user"] * (P ** 2).sum() + cfg["lambda_item"] * (Q ** 2).sum())


def planted(seed: int, groups=2, users=20, items=15, density=0.4):
    """(user ids, item ids) of `groups` disjoint blocks of users x items with
    random entries inside each block; every user and every item of a block appears at least once"""
    rng = np.random.default_rng(seed)
    pairs = []
    for g in range(groups):
        mask = rng.random((users, items)) < density
        mask[np.arange(users), rng.integers(0, items, users)] = True
        mask[rng.integers(0, users, items), np.arange(items)] = True
        pairs += [(f"u{g}-{u}", f"i{g}-{i}") for u in range(users) for i in range(items) if mask[u, i]]
    order = rng.permutation(len(pairs))
    us, its = [pairs[k][0] for k in order], [pairs[k][1] for k in order]
    return us, its


# the planted case of the CPU and GPU tests: chosen so that the restatement alone passes (tests/test_als_cpu.py)
PLANTED = dict(seed=4, density=0.4, K=8, iterations=20, init_seed=9)


def planted_neighbours_hold(items, Q, n=5):
    """every item's n nearest neighbours by cosine distance (itself excluded) lie in its own group"""
    group = np.array([i.split("-")[0] for i in items])
    unit = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    dist = 1.0 - unit @ unit.T
    np.fill_diagonal(dist, np.inf)
    near = np.argsort(dist, axis=1, kind="stable")[:, :n]
    return bool((group[near] == group[:, None]).all())

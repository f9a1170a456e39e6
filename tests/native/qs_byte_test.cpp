// Host emulation of the bit-vector scorer's BYTE-MODE tree step (score_qs.hip qs_score_byte_split_kernel, image: forest.hpp
// PackedForestQS::bnodes), bit for bit: cells clamped to 255 (v_pk_min_u16), one v_pk_sub_i16 per node (16-bit wraparound),
// (k from the low half of the node word for both rows), the A ladder over slots [0, a) and the B ladder over [x, 15) (v_and_or_b32), the v_perm_b32 merge, the categorical nodes of
// the side list on their UNCLAMPED cells, the exit leaf by ctz.  Every exit leaf is checked against the 16-bit QuickScorer rule
// on the `nodes` image (the unchanged kernels' step) and against a plain walk of the tree in bin space.
//   g++ -std=c++17 -I metarank_amd/csrc tests/native/qs_byte_test.cpp metarank_amd/csrc/forest.cpp && ./a.out
// Prints one line per case and "ALL OK"; exits 1 at the first mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "forest.hpp"

using namespace mrk;

namespace {

std::mt19937_64 rng(12345);
int urand(int n) { return (int)(rng() % (uint64_t)n); }

uint32_t pk_sub_i16(uint32_t a, uint32_t b) {  // v_pk_sub_i16: two independent 16-bit lanes, wraparound
  const uint32_t lo = (a - b) & 0xffffu;
  const uint32_t hi = ((a >> 16) - (b >> 16)) & 0xffffu;
  return lo | (hi << 16);
}
uint32_t pk_ashr15(uint32_t a) {  // v_pk_ashrrev_i16 15
  const uint32_t lo = (a & 0x8000u) ? 0xffffu : 0u, hi = (a & 0x80000000u) ? 0xffffu : 0u;
  return lo | (hi << 16);
}
uint32_t pk_min_u16(uint32_t a, uint32_t b) {
  const uint32_t lo = std::min(a & 0xffffu, b & 0xffffu), hi = std::min(a >> 16, b >> 16);
  return lo | (hi << 16);
}
uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel) {  // v_perm_b32 for selector bytes 0-7: bytes of {s0, s1}
  const uint64_t v = ((uint64_t)s0 << 32) | s1;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t b = (sel >> (8 * i)) & 0xffu;
    if (b > 7) { fprintf(stderr, "selector byte out of range\n"); exit(2); }
    r |= (uint32_t)((v >> (8 * b)) & 0xffu) << (8 * i);
  }
  return r;
}
int ctz32(uint32_t v) { return v ? __builtin_ctz(v) : 32; }

// LightGBM categorical rule (qs_device.hpp qs_cat_pair<true>): a member goes left; NaN / negative / unknown go right
uint32_t cat_pair(const PackedForestQS &pf, const QsCatNode &cn, uint32_t cc) {
  uint32_t removed = 0;
  for (int h = 0; h < 2; ++h) {
    const uint32_t cat = (cc >> (16 * h)) & 0xffffu, w = cat >> 5;
    bool in = false;
    if (cat < QS_CAT_BEYOND && w < cn.bits_words) in = (pf.cat_bits[cn.bits_begin + w] >> (cat & 31)) & 1u;
    if (!in) removed |= cn.mm & (0xffffu << (16 * h));
  }
  return removed;
}

struct Checker {
  const Forest &f;
  const PackedForestQS &pf;
  long checked = 0;
  // cells: per view, two rows (lo / hi half)
  bool tree(int ti, const std::vector<uint32_t> &cells) {
    const uint32_t *nd = pf.nodes.data() + (size_t)ti * QS_TREE_WORDS;
    const uint32_t *bd = pf.bnodes.data() + (size_t)ti * QS_BYTE_TREE_WORDS;
    uint32_t catm = 0;
    const uint32_t catw = nd[QS_SLOTS - 1];
    if (bd[QS_SLOTS - 1] != catw) return fail(ti, "categorical word differs between the images");
    for (uint32_t j = 0; j < (catw >> 24); ++j) {
      const QsCatNode &cn = pf.cat_nodes[(catw & 0xffffffu) + j];
      catm |= cat_pair(pf, cn, cells[cn.view_dl & 0xffffu]);
    }
    // 16-bit rule (the `nodes` image, unclamped cells)
    uint32_t acc16 = catm;
    for (int s = 0; s < QS_SLOTS - 1; ++s) {
      const uint32_t mv = nd[QS_SLOTS + s];
      acc16 |= pk_ashr15(pk_sub_i16(nd[s], cells[mv >> 24])) & ((mv & 0xffffu) * 0x10001u);
    }
    // byte mode (the `bnodes` image, slab cells clamped to 255)
    const uint32_t x = bd[2 * QS_SLOTS - 1] & 0xffu, a = (bd[2 * QS_SLOTS - 1] >> 8) & 0xffu;
    if (x > a || a > (uint32_t)QS_SLOTS - 1 || (bd[2 * QS_SLOTS - 1] >> 16)) return fail(ti, "bad counts");
    uint32_t d[QS_SLOTS - 1];
    const uint32_t *ma = bd + QS_SLOTS, *mb = bd + 2 * QS_SLOTS;
    for (int s = 0; s < QS_SLOTS - 1; ++s) {
      const uint32_t kv = bd[s], view = kv >> 24;
      if (kv & 0x00ffff00u) return fail(ti, "k word: bits 8-23 not zero");
      if (view >= pf.views.size()) return fail(ti, "view out of range");
      if ((kv & 0xffu) > QS_BYTE_KMAX) return fail(ti, "k out of range");
      if ((kv >> 16) != (view << 8)) return fail(ti, "M0 (word >> 16) is not the view's offset");
      // v_pk_sub_i16 d, kv, cell op_sel_hi:[0,1]: the low half of kv (k) for both rows
      d[s] = pk_sub_i16((kv & 0xffffu) * 0x10001u, pk_min_u16(cells[view], 0x00ff00ffu));
      if ((ma[s] | mb[s]) & 0x00ff00ffu) return fail(ti, "mask bits outside the high bytes");
    }
    uint32_t acc_a = 0, acc_b = 0;
    for (uint32_t s = 0; s < a; ++s) acc_a |= d[s] & ma[s];
    for (uint32_t s = x; s < (uint32_t)QS_SLOTS - 1; ++s) acc_b |= d[s] & mb[s];
    // every mask outside the ladders must be zero: the kernel's guarded blocks may run past a ladder's bound
    for (uint32_t s = a; s < (uint32_t)QS_SLOTS - 1; ++s)
      if (ma[s]) return fail(ti, "A mask beyond the A ladder");
    for (uint32_t s = 0; s < x; ++s)
      if (mb[s]) return fail(ti, "B mask before the B ladder");
    const uint32_t accb = perm_b32(acc_b, acc_a, 0x07030501u) | catm;
    // plain walk in bin space
    const Tree &t = f.trees[(size_t)ti];
    int want[2];
    for (int h = 0; h < 2; ++h) {
      int pos = 0;
      if (!t.feat.empty()) {
        // leaf positions: in-order numbering of the leaves; walk to the exit and count the leaves left of it
        std::function<int(int)> count = [&](int c) -> int { return c < 0 ? 1 : count(t.left[c]) + count(t.right[c]); };
        int n = 0;
        for (;;) {
          const size_t i = (size_t)n;
          bool left;
          const int kind_view = view_of(ti, (int)i);
          const uint32_t cell = (cells[kind_view] >> (16 * h)) & 0xffffu;
          if (t.flags[i] & NF_CATEGORICAL) {
            const uint32_t w = cell >> 5;
            left = cell < QS_CAT_BEYOND && w < t.cat_words[i] && ((f.cat_bits[t.cat_begin[i] + w] >> (cell & 31)) & 1u);
          } else {
            left = cell <= kbin(ti, (int)i);
          }
          const int c = left ? t.left[i] : t.right[i];
          if (!left) pos += count(t.left[i]);
          if (c < 0) break;
          n = c;
        }
      }
      want[h] = pos;
    }
    const int q16[2] = {ctz32(~acc16 & 0xffffu), ctz32((~acc16) >> 16)};
    const int qb[2] = {ctz32(~accb & 0xffffu), ctz32((~accb) >> 16)};
    ++checked;
    for (int h = 0; h < 2; ++h)
      if (q16[h] != want[h] || qb[h] != want[h]) {
        fprintf(stderr, "tree %d row %d: walk %d, 16-bit rule %d, byte mode %d (x %u a %u)\n", ti, h, want[h], q16[h], qb[h], x, a);
        return false;
      }
    return true;
  }
  bool fail(int ti, const char *why) {
    fprintf(stderr, "tree %d: %s\n", ti, why);
    return false;
  }
  // the view a node reads and its threshold index, recovered from the images' construction rules
  int view_of(int ti, int i) {
    const Tree &t = f.trees[(size_t)ti];
    for (size_t v = 0; v < pf.views.size(); ++v)
      if (pf.views[v].feature == t.feat[(size_t)i] && pf.views[v].kind == kind(t, (size_t)i)) return (int)v;
    fprintf(stderr, "no view\n");
    exit(2);
  }
  static int kind(const Tree &t, size_t i) {
    const uint8_t fl = t.flags[i];
    if (fl & NF_CATEGORICAL) return QV_CAT;
    const bool dl = (fl & NF_DEFAULT_LEFT) != 0;
    if (fl & NF_MISS_ZERO) return dl ? QV_MISS_LEFT : QV_MISS_RIGHT;
    if (fl & NF_MISS_NAN) return dl ? QV_NAN_LEFT : QV_NAN_RIGHT;
    return QV_NAN_ZERO;
  }
  uint32_t kbin(int ti, int i) {
    const Tree &t = f.trees[(size_t)ti];
    const QsFeature &q = pf.feats[(size_t)t.feat[(size_t)i]];
    const double *t0 = pf.thr.data() + q.thr_off, *t1 = t0 + q.thr_len;
    return (uint32_t)(std::lower_bound(t0, t1, t.thr[(size_t)i]) - t0);
  }
};

// ---- forests
struct Builder {
  Forest f;
  std::vector<std::vector<double>> pools;  // per feature: the thresholds a node may pick
  bool with_cat = false;
  explicit Builder(int n_features, int thresholds_per_feature) {
    f.backend = Backend::LightGBM;
    f.n_features = n_features;
    for (int j = 0; j < n_features; ++j) {
      std::vector<double> p;
      for (int k = 0; k < thresholds_per_feature; ++k) p.push_back(k * 0.5 - 3.0 + j);
      pools.push_back(p);
    }
  }
  // shape: a function that returns the tree's left / right arrays for `nl` leaves
  void add(const std::vector<int32_t> &left, const std::vector<int32_t> &right) {
    Tree t;
    const size_t nn = left.size();
    t.left = left;
    t.right = right;
    for (size_t i = 0; i < nn; ++i) {
      const int ft = urand(f.n_features);
      t.feat.push_back(ft);
      uint8_t fl = 0;
      const int r = urand(7);
      if (r == 1) fl = NF_MISS_NAN;
      else if (r == 2) fl = NF_MISS_NAN | NF_DEFAULT_LEFT;
      else if (r == 3) fl = NF_MISS_ZERO;
      else if (r == 4) fl = NF_MISS_ZERO | NF_DEFAULT_LEFT;
      if (with_cat && urand(8) == 0) {
        fl = NF_CATEGORICAL;
        t.feat.back() = f.n_features - 1;  // the last column is categorical
        t.cat_begin.push_back((uint32_t)f.cat_bits.size());
        const uint32_t words = 1 + (uint32_t)urand(3);
        t.cat_words.push_back(words);
        for (uint32_t w = 0; w < words; ++w) f.cat_bits.push_back((uint32_t)rng());
        t.thr.push_back(0.0);
      } else {
        if (with_cat && ft == f.n_features - 1) t.feat.back() = 0;
        const auto &p = pools[(size_t)t.feat.back()];
        t.thr.push_back(p[(size_t)urand((int)p.size())]);
        t.cat_begin.push_back(0);
        t.cat_words.push_back(0);
      }
      t.flags.push_back(fl);
    }
    for (size_t l = 0; l < nn + 1; ++l) t.leaf.push_back((double)l);
    f.trees.push_back(t);
  }
  // every threshold of feature `ft`'s pool used at least once (so that the column's table has all of them)
  void cover(int ft) {
    for (size_t k = 0; k < pools[(size_t)ft].size(); ++k) {
      Tree t;
      t.feat = {ft};
      t.thr = {pools[(size_t)ft][k]};
      t.flags = {0};
      t.left = {~0};
      t.right = {~1};
      t.cat_begin = {0};
      t.cat_words = {0};
      t.leaf = {0.0, 1.0};
      f.trees.push_back(t);
    }
  }
};

// random binary tree with nl leaves: node ids in creation order (root 0)
void random_shape(int nl, std::vector<int32_t> &left, std::vector<int32_t> &right) {
  left.clear();
  right.clear();
  int leaves = 0;
  std::function<int32_t(int)> build = [&](int n) -> int32_t {
    if (n == 1) return ~(leaves++);
    const int id = (int)left.size();
    left.push_back(0);
    right.push_back(0);
    const int nl_left = 1 + urand(n - 1);
    const int32_t l = build(nl_left);
    const int32_t r = build(n - nl_left);
    left[(size_t)id] = l;
    right[(size_t)id] = r;
    return id;
  };
  build(nl);
}
void comb(int nl, bool left_comb, std::vector<int32_t> &left, std::vector<int32_t> &right) {
  left.assign((size_t)nl - 1, 0);
  right.assign((size_t)nl - 1, 0);
  int leaf = 0;
  for (int i = 0; i < nl - 1; ++i) {
    const int32_t next = i + 1 < nl - 1 ? i + 1 : ~(leaf++);
    if (left_comb) {
      left[(size_t)i] = next;
      right[(size_t)i] = ~(leaf++);
    } else {
      left[(size_t)i] = ~(leaf++);
      right[(size_t)i] = next;
    }
  }
}

uint32_t random_cell(const PackedForestQS &pf, size_t v) {
  if (pf.views[v].kind == QV_CAT) {
    const int r = urand(10);
    return r == 0 ? QS_CAT_NAN : r == 1 ? QS_CAT_BEYOND : (uint32_t)urand(100);
  }
  const int r = urand(20);
  return r == 0 ? (uint32_t)QS_RIGHT : r == 1 ? 0u : (uint32_t)urand(300);  // beyond 255 too: a column may have more thresholds than its nodes use
}

bool run_case(const char *name, Builder &b, bool expect_byte, int sweeps) {
  const PackedForestQS pf = pack_forest_qs(b.f, b.f.n_features);
  if (!pf.ok) {
    printf("%s: pack failed: %s\n", name, pf.why.c_str());
    return false;
  }
  if (pf.byte_ok != expect_byte) {
    printf("%s: byte mode %s, expected %s\n", name, pf.byte_ok ? "on" : "off", expect_byte ? "on" : "off");
    return false;
  }
  if (!pf.byte_ok) {
    printf("%s: byte mode refused, as expected (%zu tile columns)\n", name, pf.views.size());
    return true;
  }
  if (pf.bnodes.size() != (size_t)(pf.n_trees + 1) * QS_BYTE_TREE_WORDS) {
    printf("%s: bnodes size\n", name);
    return false;
  }
  for (int w = 0; w < QS_BYTE_TREE_WORDS; ++w)
    if (pf.bnodes[(size_t)pf.n_trees * QS_BYTE_TREE_WORDS + w]) {
      printf("%s: the trailing tree is not all zero\n", name);
      return false;
    }
  Checker ck{b.f, pf};
  int max_z = 0;
  double sum_z = 0;
  for (int ti = 0; ti < pf.n_trees; ++ti) {
    const uint32_t cw = pf.bnodes[(size_t)ti * QS_BYTE_TREE_WORDS + 2 * QS_SLOTS - 1];
    const int z = (int)((cw >> 8) & 0xff) - (int)(cw & 0xff);
    max_z = std::max(max_z, z);
    sum_z += z;
    std::vector<uint32_t> cells(pf.views.size());
    const Tree &t = b.f.trees[(size_t)ti];
    for (int rep = 0; rep < sweeps; ++rep) {
      for (size_t v = 0; v < cells.size(); ++v) cells[v] = random_cell(pf, v) | (random_cell(pf, v) << 16);
      if (!ck.tree(ti, cells)) return false;
      // every node's view through every cell value in [0, 255] and 0x7FFF (a missing value sent right), both rows
      for (size_t i = 0; i < t.feat.size(); ++i) {
        const int v = ck.view_of(ti, (int)i);
        const uint32_t keep = cells[(size_t)v];
        for (uint32_t c = 0; c <= 256; ++c) {
          const uint32_t cell = c == 256 ? (uint32_t)QS_RIGHT : c;
          cells[(size_t)v] = cell | ((c == 256 ? 0u : 255u - c) << 16);
          if (!ck.tree(ti, cells)) return false;
        }
        cells[(size_t)v] = keep;
      }
    }
  }
  printf("%s: %d trees, %zu tile columns, %ld tree steps checked, crossing nodes per tree mean %.2f max %d\n", name, pf.n_trees,
         pf.views.size(), ck.checked, sum_z / pf.n_trees, max_z);
  return true;
}

}  // namespace

int main() {
  std::vector<int32_t> l, r;
  bool ok = true;
  {
    Builder b(6, 40);
    for (int i = 0; i < 300; ++i) {
      random_shape(16, l, r);
      b.add(l, r);
    }
    ok = ok && run_case("random 16-leaf trees", b, true, 2);
  }
  {
    Builder b(5, 30);
    for (int i = 0; i < 300; ++i) {
      random_shape(1 + urand(16), l, r);
      b.add(l, r);
    }
    ok = ok && run_case("random trees of 1-16 leaves", b, true, 2);
  }
  {
    Builder b(4, 20);
    for (int nl : {16, 9, 8, 2}) {
      comb(nl, true, l, r);
      b.add(l, r);
      comb(nl, false, l, r);
      b.add(l, r);
    }
    ok = ok && run_case("left and right combs", b, true, 4);
  }
  {
    Builder b(3, 255);  // k up to 254 on every column
    for (int ft = 0; ft < 3; ++ft) b.cover(ft);
    for (int i = 0; i < 100; ++i) {
      random_shape(16, l, r);
      b.add(l, r);
    }
    ok = ok && run_case("255 thresholds per column (k = 254)", b, true, 1);
  }
  {
    Builder b(5, 30);
    b.with_cat = true;
    for (int i = 0; i < 300; ++i) {
      random_shape(2 + urand(15), l, r);
      b.add(l, r);
    }
    ok = ok && run_case("categorical nodes", b, true, 2);
  }
  {
    Builder b(3, 256);  // one threshold index reaches 255
    b.cover(1);
    random_shape(16, l, r);
    b.add(l, r);
    ok = ok && run_case("256 thresholds on a column", b, false, 1);
  }
  if (!ok) return 1;
  printf("ALL OK\n");
  return 0;
}

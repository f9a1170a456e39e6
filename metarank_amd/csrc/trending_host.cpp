// Host half of the trending recommender.  See trending_host.hpp.
#include "trending_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "duration.hpp"
#include "json.hpp"

namespace mrk {

int64_t TrendingConfig::total_days() const {
  int64_t d = 0;
  for (auto &w : weights) d += w.days;
  return d;
}

int TrendingConfig::weight_of(const char *type) const {
  for (size_t i = 0; i < weights.size(); ++i)
    if (weights[i].interaction == type) return (int)i;
  return -1;
}

TrendingConfig trending_parse_config(const char *json, size_t len) {
  auto bad = [](const std::string &m) -> void { throw StatusError(MRK_ERR_PARSE, "trending config: " + m); };
  json::Value root;
  try {
    root = json::parse(json, len);
  } catch (const std::exception &e) {
    bad(e.what());
  }
  if (!root.is_object()) bad("not an object");
  const json::Value *ws = root.find("weights");
  if (!ws || !ws->is_array()) bad("missing 'weights' list");
  TrendingConfig cfg;
  for (auto &o : ws->arr) {
    if (!o.is_object()) bad("a weight is not an object");
    TrendingWeight w;
    const json::Value *tpe = o.find("interaction");
    if (!tpe || !tpe->is_string()) bad("a weight without 'interaction'");
    w.interaction = tpe->str;
    auto number = [&](const char *key, double &out) {
      const json::Value *v = o.find(key);
      if (!v || v->is_null()) return;   // Option[Double]: the default stays
      if (!v->is_number()) bad(std::string("'") + key + "' of weight '" + w.interaction + "' is not a number");
      out = v->as_double();
    };
    number("weight", w.weight);
    number("decay", w.decay);
    if (const json::Value *win = o.find("window"))
      if (!win->is_null()) {
        if (!win->is_string() || !parse_duration_ms(win->str, w.window_ms)) bad("duration is in wrong format: " + (win->is_string() ? win->str : std::string("<not a string>")));
        w.days = w.window_ms / TRENDING_DAY_MS;
      }
    if (cfg.weight_of(w.interaction.c_str()) >= 0)
      throw StatusError(MRK_ERR_UNSUPPORTED, "trending config: two weights name the interaction '" + w.interaction + "'");
    cfg.weights.push_back(std::move(w));
  }
  return cfg;
}

std::vector<double> trending_pow_table(double decay, int64_t days) {
  std::vector<double> t((size_t)std::max<int64_t>(days, 0));
  for (size_t i = 0; i < t.size(); ++i) t[i] = std::pow(decay, (double)i);
  return t;
}

uint32_t TrendingStream::intern(const char *id) {
  auto it = index_of.find(id);
  if (it != index_of.end()) return it->second;
  const uint32_t k = (uint32_t)ids.size();
  ids.emplace_back(id);
  index_of.emplace(ids.back(), k);
  return k;
}

std::vector<int32_t> trending_check_call(const TrendingConfig &cfg, const TrendingStream &st, const char *const *item_ids,
                                         const char *const *type_names, int n_types, const int32_t *type_idx,
                                         const int64_t *ts_ms, int64_t n) {
  need(n >= 0, "trending: negative interaction count");
  need(n_types >= 0, "trending: negative type count");
  need(n == 0 || (item_ids && type_idx && ts_ms), "null item_ids / type_idx / ts_ms");
  need(n_types == 0 || type_names, "null type_names");
  if (n > TRENDING_MAX_INTERACTIONS - st.interactions)
    throw StatusError(MRK_ERR_UNSUPPORTED, "trending: more than 2^31 - 1 interactions in one fit");
  std::vector<int32_t> weight_of((size_t)n_types);
  for (int t = 0; t < n_types; ++t) {
    need(type_names[t] != nullptr, "null type name");
    weight_of[(size_t)t] = cfg.weight_of(type_names[t]);
  }
  for (int64_t i = 0; i < n; ++i) {
    need(item_ids[i] != nullptr, "null item id");
    if (type_idx[i] < 0 || type_idx[i] >= n_types)
      throw StatusError(MRK_ERR_INVALID_ARG, "trending: type_idx[" + std::to_string(i) + "] = " + std::to_string(type_idx[i]) + " is outside the call's " +
                                                   std::to_string(n_types) + " type names");
  }
  return weight_of;
}

namespace {

void put_i32(std::vector<uint8_t> &o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s));
}

struct Rd {
  const uint8_t *p, *end;
  void need(size_t n) {
    if ((size_t)(end - p) < n) throw StatusError(MRK_ERR_PARSE, "trending model: truncated");
  }
  int32_t i32() {
    need(4);
    const uint32_t v = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    p += 4;
    return (int32_t)v;
  }
  // DataInput.readUTF: u16 byte length + modified UTF-8, returned as the raw bytes (codec.cpp's convention)
  std::string utf() {
    need(2);
    const size_t n = (size_t)p[0] << 8 | p[1];
    p += 2;
    need(n);
    std::string s((const char *)p, n);
    p += n;
    return s;
  }
  double f64() {
    need(8);
    uint64_t u = 0;
    for (int i = 0; i < 8; ++i) u = (u << 8) | p[i];
    p += 8;
    double d;
    memcpy(&d, &u, 8);
    return d;
  }
};

}  // namespace

std::vector<uint8_t> trending_save(const TrendingModel &m) {
  std::vector<uint8_t> o;
  size_t bytes = 8;
  for (auto &id : m.ids) {
    if (id.size() > 65535)
      throw StatusError(MRK_ERR_UNSUPPORTED, "trending model: an item id of " + std::to_string(id.size()) + " bytes does not fit writeUTF's 65535");
    bytes += 2 + id.size() + 8;
  }
  o.reserve(bytes);
  put_i32(o, 1);
  put_i32(o, (uint32_t)m.ids.size());
  for (size_t i = 0; i < m.ids.size(); ++i) {
    const std::string &id = m.ids[i];
    o.push_back((uint8_t)(id.size() >> 8));
    o.push_back((uint8_t)id.size());
    o.insert(o.end(), id.begin(), id.end());
    uint64_t u;
    memcpy(&u, &m.scores[i], 8);
    for (int s = 56; s >= 0; s -= 8) o.push_back((uint8_t)(u >> s));
  }
  return o;
}

TrendingModel trending_load(const uint8_t *bytes, size_t len) {
  Rd r{bytes, bytes + len};
  const int32_t version = r.i32();
  if (version != 1) throw StatusError(MRK_ERR_UNSUPPORTED, "unsupported format " + std::to_string(version));
  const int32_t size = r.i32();
  if (size <= 0) throw StatusError(MRK_ERR_PARSE, "trending model: no items found");
  if ((size_t)size > (size_t)(r.end - r.p) / 10)   // an item takes 10 bytes at least: the count must not size an allocation
    throw StatusError(MRK_ERR_PARSE, "trending model: truncated (" + std::to_string(size) + " items do not fit " + std::to_string(r.end - r.p) + " bytes)");
  TrendingModel m;
  m.ids.reserve((size_t)size);
  m.scores.reserve((size_t)size);
  for (int32_t i = 0; i < size; ++i) {
    m.ids.push_back(r.utf());
    m.scores.push_back(r.f64());
  }
  if (r.p != r.end) throw StatusError(MRK_ERR_PARSE, "trending model: " + std::to_string(r.end - r.p) + " bytes after the last item");
  return m;
}

int trending_predict_n(const TrendingModel &m, int count) {
  if (count <= 0) throw StatusError(MRK_ERR_INVALID_ARG, "count should be greater than 0");
  return (int)std::min<int64_t>(count, (int64_t)m.ids.size());
}

}  // namespace mrk

// Host half of the similar-items fit (csrc/als_host.cpp) without HIP: the config decoder and its refusals, interning in order of
// first appearance, duplicate collapse, CSR / CSC, the confidences, the row orders and the generator, on the edge inputs: no pairs,
// one pair, all pairs equal, ids of length 0 and 65 536, null ids.  Built with ASan + UBSan by tests/test_als_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mrk.h"
#include "als_host.hpp"

using namespace mrk;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

template <typename F>
static int status_of(F &&f) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    return e.status;
  }
}

static AlsConfig parse(const std::string &s) { return als_parse_config(s.c_str(), s.size()); }

static void add(AlsStream &st, const std::vector<const char *> &u, const std::vector<const char *> &i) { st.add(u.data(), i.data(), (int64_t)u.size()); }

int main() {
  {  // the decoder: ALSConfig's defaults (ALSRecImpl.scala:46-54), itemRef honoured and itemReg ignored (:66), floats widened
    const AlsConfig d = parse("{}");
    CHECK(d.iterations == 100 && d.factors == 100);
    CHECK(bits(d.lambda_user()) == bits((double)0.01f) && bits(d.lambda_item()) == bits((double)0.01f));
    CHECK(d.lambda_user() != 0.01);
    const AlsConfig c = parse(R"({"interactions":["click"],"iterations":7,"factors":3,"userReg":0.1,"itemReg":0.5,"itemRef":0.25,"store":{"type":"hnsw"},"selector":null})");
    CHECK(c.iterations == 7 && c.factors == 3 && bits(c.lambda_user()) == bits((double)0.1f) && c.lambda_item() == 0.25);
    CHECK(bits(parse(R"({"itemReg":0.5})").lambda_item()) == bits((double)0.01f));
    CHECK(parse(R"({"iterations":null,"factors":null,"userReg":null,"itemRef":null,"interactions":null})").factors == 100);
    CHECK(status_of([] { parse("{\"factors\":3"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse("[]"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"factors":"3"})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"factors":2.5})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"userReg":"x"})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"interactions":"click"})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"interactions":[1]})"); }) == MRK_ERR_PARSE);
    CHECK(status_of([] { parse(R"({"factors":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"iterations":0})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([] { parse(R"({"iterations":-4})"); }) == MRK_ERR_INVALID_ARG);
    CHECK(parse(R"({"factors":1000})").factors == 1000);   // (the bound is the fit's)
  }
  {  // no pairs
    AlsStream st;
    st.add(nullptr, nullptr, 0);
    CHECK(st.pairs.empty() && st.distinct_pairs() == 0);
    CHECK(status_of([&] { st.add(nullptr, nullptr, -1); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { st.add(nullptr, nullptr, 1); }) == MRK_ERR_INVALID_ARG);
  }
  {  // one pair: c_0 = w0 exactly (p = 1, Z = 1)
    AlsStream st;
    add(st, {"u"}, {"i"});
    const AlsProblem pr = als_build_problem(st);
    CHECK(pr.users == 1 && pr.items == 1 && pr.nnz == 1);
    CHECK(pr.u_off == std::vector<int32_t>({0, 1}) && pr.i_off == std::vector<int32_t>({0, 1}) && pr.u_idx[0] == 0 && pr.i_idx[0] == 0);
    CHECK(pr.conf.size() == 1 && pr.conf[0] == 128.0);
  }
  {  // all pairs equal
    AlsStream st;
    for (int k = 0; k < 3; ++k) add(st, {"u", "u", "u"}, {"i", "i", "i"});
    CHECK(st.pairs.size() == 9 && st.distinct_pairs() == 1);
    const AlsProblem pr = als_build_problem(st);
    CHECK(pr.users == 1 && pr.items == 1 && pr.nnz == 1 && pr.u_idx.size() == 1);
  }
  {  // interning order, the cut into calls, CSR / CSC, a null id appends nothing, ids of length 0 and 65 536
    const std::string long_id(65536, 'x');
    AlsStream a, b;
    add(a, {"u2", "u0", "u2", "", "u0", "u2"}, {"b", "a", "a", long_id.c_str(), "", "b"});
    add(b, {"u2"}, {"b"});
    CHECK(status_of([&] { add(b, {"u0", nullptr}, {"a", "a"}); }) == MRK_ERR_INVALID_ARG);
    CHECK(status_of([&] { add(b, {"zz", "u0"}, {"a", nullptr}); }) == MRK_ERR_INVALID_ARG);
    CHECK(b.pairs.size() == 1 && b.users.size() == 1 && b.items.size() == 1);
    add(b, {"u0", "u2", ""}, {"a", "a", long_id.c_str()});
    add(b, {"u0", "u2"}, {"", "b"});
    CHECK(a.users == b.users && a.items == b.items && a.pairs == b.pairs);
    CHECK(a.users == std::vector<std::string>({"u2", "u0", ""}));
    CHECK(a.items.size() == 4 && a.items[0] == "b" && a.items[1] == "a" && a.items[2] == long_id && a.items[3].empty());
    const AlsProblem pr = als_build_problem(a);
    CHECK(pr.nnz == 5 && a.distinct_pairs() == 5);
    CHECK(pr.u_off == std::vector<int32_t>({0, 2, 4, 5}) && pr.u_idx == std::vector<int32_t>({0, 1, 1, 3, 2}));
    CHECK(pr.i_off == std::vector<int32_t>({0, 1, 3, 4, 5}) && pr.i_idx == std::vector<int32_t>({0, 0, 1, 2, 1}));
    CHECK(pr.u_order == std::vector<int32_t>({0, 1, 2}) && pr.i_order == std::vector<int32_t>({1, 0, 2, 3}));
    double z = 0.0;
    for (int n : {1, 2, 1, 1}) z = z + std::pow((double)n / 5.0, 0.4);
    CHECK(bits(pr.conf[1]) == bits(128.0 * std::pow(2.0 / 5.0, 0.4) / z) && bits(pr.conf[0]) == bits(128.0 * std::pow(1.0 / 5.0, 0.4) / z));
    printf("interned: users=%s,%s,[%zu] items=%s,%s,[%zu],[%zu]\n", a.users[0].c_str(), a.users[1].c_str(), a.users[2].size(), a.items[0].c_str(),
           a.items[1].c_str(), a.items[2].size(), a.items[3].size());
  }
  {  // the generator: a function of (seed, matrix, row, column) alone; about N(0, 0.01^2)
    std::vector<double> m(50 * 40), again(50 * 40), other(50 * 40), items(50 * 40), sub(3 * 7);
    als_init_matrix(7, 0, 50, 40, m.data());
    als_init_matrix(7, 0, 50, 40, again.data());
    als_init_matrix(8, 0, 50, 40, other.data());
    als_init_matrix(7, 1, 50, 40, items.data());
    als_init_matrix(7, 0, 3, 7, sub.data());
    CHECK(memcmp(m.data(), again.data(), m.size() * 8) == 0);
    CHECK(memcmp(m.data(), other.data(), m.size() * 8) != 0 && memcmp(m.data(), items.data(), m.size() * 8) != 0);
    CHECK(bits(sub[1 * 7 + 5]) == bits(m[1 * 40 + 5]) && bits(m[2 * 40 + 3]) == bits(als_init_value(7, 0, 2, 3)));
    double mean = 0.0, var = 0.0;
    for (double v : m) mean += v / (double)m.size();
    for (double v : m) var += (v - mean) * (v - mean) / (double)m.size();
    CHECK(std::fabs(mean) < 0.001 && std::sqrt(var) > 0.009 && std::sqrt(var) < 0.011);   // 2 000 samples: s.e. of the mean 0.00022, of the s.d. 0.00016
    for (double v : m) CHECK(std::isfinite(v));
    als_init_matrix(7, 0, 0, 40, nullptr);
  }
  if (failures == 0) printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}

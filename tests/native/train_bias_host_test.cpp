// Host half of step 3b (position_bias) of the LambdaMART fit, csrc/train_host.cpp without HIP: the key's decoder and its refusals, the
// cost table and the update of the factors.  Built with ASan + UBSan by tests/test_train_bias_cpu.py; runs on the CPU only.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mrk.h"
#include "train_host.hpp"

using namespace mrk;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static int status_of(const std::string &s) {
  try {
    train_parse_config(s.c_str(), s.size());
    return MRK_OK;
  } catch (const StatusError &e) {
    return e.status;
  }
}

int main() {
  {  // the decoder
    const std::string none = R"({"position_bias":null})", d = R"({"position_bias":{"norm":null}})";
    const std::string x = R"({"backend":"xgboost","position_bias":{"positions":4096,"norm":0,"x":null}})";
    CHECK(!train_parse_config("{}", 2).position_bias && !train_parse_config(none.c_str(), none.size()).position_bias);
    const TrainConfig dflt = train_parse_config(d.c_str(), d.size());
    CHECK(dflt.position_bias && dflt.bias_positions == 32 && dflt.bias_norm == 1.0);
    CHECK(status_of(R"({"backend":"xgboost","position_bias":{"positions":4096,"norm":0}})") == MRK_OK);
    CHECK(status_of(x) == MRK_ERR_PARSE);   // an unknown key inside, even a null one
    CHECK(status_of(R"({"position_bias":true})") == MRK_ERR_PARSE && status_of(R"({"position_bias":[]})") == MRK_ERR_PARSE);
    CHECK(status_of(R"({"position_bias":{"positions":"8"}})") == MRK_ERR_PARSE && status_of(R"({"position_bias":{"positions":1.5}})") == MRK_ERR_PARSE);
    CHECK(status_of(R"({"position_bias":{"norm":"1"}})") == MRK_ERR_PARSE);
    CHECK(status_of(R"({"position_bias":{"positions":0}})") == MRK_ERR_INVALID_ARG && status_of(R"({"position_bias":{"positions":4097}})") == MRK_ERR_INVALID_ARG);
    CHECK(status_of(R"({"position_bias":{"norm":-0.5}})") == MRK_ERR_INVALID_ARG && status_of(R"({"position_bias":{"norm":1e999}})") != MRK_OK);
    CHECK(status_of(R"({"debias":true,"position_bias":{}})") == MRK_ERR_UNSUPPORTED);
  }
  {  // L[t] = log1p(exp(-sigma * x)) under the sigmoid table's index: with rho = 1 / (1 + exp(sigma * x)), exp(-L) = 1 - rho
    const SigmoidTable s = train_sigmoid_table(2.0);
    const std::vector<double> L = train_cost_table(2.0);
    CHECK((int)L.size() == TRAIN_SIGMOID_BINS && L[0] == std::log1p(std::exp(25.0)) && L[100] > L[101] && L.back() > 0.0);
    for (int t : {0, 1, 32768, 65535}) CHECK(std::fabs(std::exp(-L[(size_t)t]) - (1.0 - s.t[(size_t)t])) < 1e-14);
  }
  {  // the update: S[0] == 0 keeps every factor; S[i] == 0 keeps that one; t[0] becomes exactly 1
    std::vector<double> t{3.0, 3.0, 3.0, 3.0};
    const int64_t none[4] = {0, 8, 0, 2}, q[4] = {8, 2, 0, 32};
    train_bias_update(none, 3, 1.0, t.data(), 4);
    CHECK(t == std::vector<double>(4, 3.0));
    train_bias_update(q, 3, 1.0, t.data(), 4);
    CHECK(t[0] == 1.0 && t[1] == std::pow(0.25, 0.5) && t[2] == 3.0 && t[3] == std::pow(4.0, 0.5));
    train_bias_update(q, -70, 0.0, t.data(), 4);   // norm 0: the ratio itself, whatever the exponent
    CHECK(t[0] == 1.0 && t[1] == 0.25 && t[2] == 3.0 && t[3] == 4.0);
  }
  if (failures) return 1;
  printf("ALL OK\n");
  return 0;
}

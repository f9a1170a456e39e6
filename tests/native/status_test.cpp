// Host test of the C ABI's error boundary (csrc/status.hpp): guard's three clauses and its fallback, need, and UnsupportedModel as
// a StatusError.  Includes status.hpp and forest.hpp only and builds with g++ alone, so it also holds that neither needs HIP.
// Built and run by tests/test_status_cpu.py under ASan + UBSan.
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>

#include "forest.hpp"
#include "status.hpp"

static std::string g_last = "untouched";
void mrk::set_last_error(const std::string &msg) { g_last = msg; }

using namespace mrk;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// the status of a body that throws `e`, and the message it left
template <typename E>
static int thrown(const E &e, std::string &msg) {
  g_last = "untouched";
  const int rc = guard([&] { throw e; });
  msg = g_last;
  return rc;
}

int main() {
  std::string msg;
  // a StatusError keeps its own status, whatever it is
  CHECK(thrown(StatusError(MRK_ERR_INVALID_ARG, "bad argument"), msg) == MRK_ERR_INVALID_ARG && msg == "bad argument");
  CHECK(thrown(StatusError(MRK_ERR_NOT_FOUND, "nothing there"), msg) == MRK_ERR_NOT_FOUND && msg == "nothing there");
  // ... also under another fallback
  g_last = "untouched";
  CHECK(guard([] { throw StatusError(MRK_ERR_DIM_MISMATCH, "too narrow"); }, MRK_ERR_DEVICE) == MRK_ERR_DIM_MISMATCH && g_last == "too narrow");
  // the loader's refusal is one of them
  CHECK(thrown(UnsupportedModel("xgboost: dart"), msg) == MRK_ERR_UNSUPPORTED && msg == "xgboost: dart");
  try {
    throw UnsupportedModel("caught by its base");
  } catch (const StatusError &e) {
    CHECK(e.status == MRK_ERR_UNSUPPORTED && std::string(e.what()) == "caught by its base");
  }
  // out of host memory: the device status, one fixed text, under either fallback
  CHECK(thrown(std::bad_alloc(), msg) == MRK_ERR_DEVICE && msg == "out of host memory");
  g_last = "untouched";
  CHECK(guard([] { throw std::bad_alloc(); }, MRK_ERR_PARSE) == MRK_ERR_DEVICE && g_last == "out of host memory");
  // anything else: the fallback, MRK_ERR_PARSE unless the caller says otherwise
  CHECK(thrown(std::runtime_error("tree has a cycle"), msg) == MRK_ERR_PARSE && msg == "tree has a cycle");
  g_last = "untouched";
  CHECK(guard([] { throw std::runtime_error("ncclAllGather failed"); }, MRK_ERR_DEVICE) == MRK_ERR_DEVICE && g_last == "ncclAllGather failed");
  // a body that returns: MRK_OK, and the last message stays what it was
  g_last = "an earlier error";
  int ran = 0;
  CHECK(guard([&] { ++ran; }) == MRK_OK && ran == 1 && g_last == "an earlier error");
  CHECK(guard([&] { ++ran; }, MRK_ERR_DEVICE) == MRK_OK && ran == 2 && g_last == "an earlier error");
  // need
  need(true, "never thrown");
  CHECK(guard([] { need(true, "never thrown"); }) == MRK_OK);
  CHECK(guard([] { need(false, "null builder"); }) == MRK_ERR_INVALID_ARG && g_last == "null builder");
  try {
    need(false, "directly");
    CHECK(false);
  } catch (const StatusError &e) {
    CHECK(e.status == MRK_ERR_INVALID_ARG && std::string(e.what()) == "directly");
  }
  if (failures) return 1;
  std::printf("ALL OK\n");
  return 0;
}

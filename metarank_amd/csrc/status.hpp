// The error boundary of the C ABI (include/mrk.h): the one exception that carries an mrk_status, and the one place where
// exceptions become status codes.  No HIP here: the *_host.cpp halves and the drivers under tests/native include this
// header and build with a plain host compiler.
#pragma once
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/mrk.h"

namespace mrk {

struct StatusError : std::runtime_error {
  int status;
  StatusError(int s, const std::string &m) : std::runtime_error(m), status(s) {}
};

void set_last_error(const std::string &msg);  // capi.cpp: what mrk_last_error() returns on the calling thread

inline void need(bool ok, const char *what) {
  if (!ok) throw StatusError(MRK_ERR_INVALID_ARG, what);
}

// Every extern "C" entry runs its body through this.  `fallback` is the status of an exception that is no StatusError:
// malformed input for the parsers behind most entries, MRK_ERR_DEVICE for the collectives (comm.cpp).
template <typename F>
int guard(F &&f, int fallback = MRK_ERR_PARSE) {
  try {
    f();
    return MRK_OK;
  } catch (const StatusError &e) {
    set_last_error(e.what());
    return e.status;
  } catch (const std::bad_alloc &) {
    set_last_error("out of host memory");
    return MRK_ERR_DEVICE;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return fallback;
  }
}

}  // namespace mrk

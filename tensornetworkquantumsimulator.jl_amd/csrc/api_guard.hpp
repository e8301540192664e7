// api_guard.hpp -- what every extern "C" entry point of libtnqs_hip.so is wrapped in (api.cpp: include/tnqs.h; debug_*.cpp: include/tnqs_debug.h):
// no C++ exception crosses the ABI, the message of a failed call is kept for tnqs_last_error() of the same thread.
#pragma once
#include <exception>
#include <new>
#include "engine.hpp"

struct tnqs_state_s { tnqs::State* s; };

namespace tnqs {
void set_last_error(const char* msg);      // api.cpp: the ONE thread-local string behind tnqs_last_error()

template <class F> int guard(F&& f) {
    try { f(); return TNQS_OK; }
    catch (const Err& e) { set_last_error(e.what()); return e.code; }
    catch (const std::bad_alloc&) { set_last_error("out of host memory"); return TNQS_ERR_HIP; }
    catch (const std::exception& e) { set_last_error(e.what()); return TNQS_ERR_INVALID; }
    catch (...) { set_last_error("unknown error"); return TNQS_ERR_INVALID; }
}
inline State* S(tnqs_handle h) { if (!h || !h->s) throw Err(TNQS_ERR_INVALID, "null handle"); return h->s; }
}  // namespace tnqs

// route.h — what cc_route_events (route.cpp) and cc_route_events_device (route_gpu.hip) share: the argument checks and
// the word in which a bad event is reported.  Both forms keep the minimum over all offending events of
//   event << 1 | kind
// (the host with a compare-exchange loop, the device with an atomicMin), so the event named in the message is the
// lowest offending one, whatever order the checks ran in.
#pragma once
#include <cstdint>

#include "engine_state.h"

namespace cc {

enum : uint32_t { kRouteTarget = 0, kRouteSession = 1 };
constexpr uint64_t kRouteNoErr = ~0ull;

constexpr uint64_t route_key(uint64_t event, uint32_t kind) { return event << 1 | kind; }

// rounds of CC_ROUTE_DIGIT_BITS that order ordinals below n_sessions: ceil(bits(n_sessions - 1) / CC_ROUTE_DIGIT_BITS)
inline uint32_t route_rounds(uint32_t n_sessions) {
  uint32_t bits = 0;
  for (uint32_t x = n_sessions ? n_sessions - 1 : 0; x; x >>= 1) ++bits;
  return (bits + CC_ROUTE_DIGIT_BITS - 1) / CC_ROUTE_DIGIT_BITS;
}

// sets the last error to "<who>: event E: <what>" and returns CC_ERR_INVALID (route.cpp)
int route_fail(const char* who, uint64_t key);

// Every check that needs no event: CC_OK, or the code after set_err.  The capacity of `out` is answered here, too.
int route_check_args(const char* who, const cc_events* in, uint64_t n_events, const uint32_t* session_of_inst,
                     const uint64_t* id_of_inst, uint32_t n_inst, uint32_t n_sessions, const cc_events* out,
                     const uint64_t* out_instance, const cc_route_dir* dir, const uint64_t* n_active);

}  // namespace cc

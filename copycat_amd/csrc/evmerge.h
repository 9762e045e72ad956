// evmerge.h — what cc_merge_events (evmerge.cpp) and cc_merge_events_device (evmerge_gpu.hip) share: the word in which
// a broken precondition is reported.  Both forms keep the minimum over all failing events of
//   rank << 34 | event << 2 | kind
// (the host with a compare-exchange loop, the device with an atomicMax of the complement), so the event named in the
// message is the lowest rank's first failing one, whatever order the checks ran in.
#pragma once
#include <cstdint>

namespace cc {

enum : uint32_t { kEvmPosRange = 0, kEvmPosOrder = 1, kEvmRowRange = 2, kEvmClaimed = 3 };

constexpr uint64_t evmerge_key(uint32_t rank, uint64_t event, uint32_t kind) {
  return (uint64_t)rank << 34 | event << 2 | kind;
}

// sets the last error to "<who>: rank R, event E: <what>" and returns CC_ERR_INVALID (evmerge.cpp)
int evmerge_fail(const char* who, uint64_t key);

}  // namespace cc

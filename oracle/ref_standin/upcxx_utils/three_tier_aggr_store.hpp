// One-rank stand-in for upcxx_utils/three_tier_aggr_store.hpp (TEST INFRASTRUCTURE ONLY): the same synchronous
// store as FlatAggrStore, there being no node or thread tier to route through.
#pragma once

#include "upcxx_utils/flat_aggr_store.hpp"

namespace upcxx_utils {

template <typename T>
class ThreeTierAggrStore : public FlatAggrStore<T> {};

}  // namespace upcxx_utils

// One-rank stand-in for upcxx_utils/flat_aggr_store.hpp (TEST INFRASTRUCTURE ONLY).
//
// An aggregating store buffers updates per target rank and ships them in batches; the target applies the update
// function to each. With one rank there is nothing to ship: update() applies the function at once, whatever the
// target rank says.
#pragma once

#include <cstdint>
#include <functional>
#include <string>

#include "upcxx_utils/log.hpp"

namespace upcxx_utils {

template <typename T>
class FlatAggrStore {
  std::function<void(T)> update_func_;

 public:
  void set_size(const std::string &, int64_t, int = 0, bool = false) {}
  template <typename F>
  void set_update_func(F f) {
    update_func_ = std::move(f);
  }
  void update(upcxx::intrank_t, T &elem) { update_func_(elem); }
  void update(upcxx::intrank_t, const T &elem) { update_func_(elem); }
  void flush_updates() {}
  void clear() {}
};

}  // namespace upcxx_utils

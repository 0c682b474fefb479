// One-rank stand-in for upcxx_utils.hpp (TEST INFRASTRUCTURE ONLY, oracle/Makefile `ref`): the umbrella header.
#pragma once

#include <chrono>
#include <string>

#include <upcxx/upcxx.hpp>

#include "upcxx_utils/flat_aggr_store.hpp"
#include "upcxx_utils/log.hpp"
#include "upcxx_utils/mem_profile.hpp"
#include "upcxx_utils/ofstream.hpp"
#include "upcxx_utils/thread_pool.hpp"
#include "upcxx_utils/three_tier_aggr_store.hpp"

namespace upcxx_utils {

// Timers: they measure, and report nothing.
class BaseTimer {
  std::chrono::steady_clock::time_point t0_{};
  double elapsed_ = 0;

 public:
  BaseTimer() = default;
  explicit BaseTimer(const std::string &) {}
  void start() { t0_ = std::chrono::steady_clock::now(); }
  void stop() { elapsed_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); }
  double get_elapsed() const { return elapsed_; }
  void done() const {}
  void done_all() const {}
};
using IntermittentTimer = BaseTimer;
using StallTimer = BaseTimer;

class BarrierTimer {
 public:
  explicit BarrierTimer(const std::string &, bool = true) {}
};

}  // namespace upcxx_utils

// One-rank stand-in for <upcxx/upcxx.hpp> (TEST INFRASTRUCTURE ONLY, oracle/Makefile `ref`).
//
// The reference's kcount sources are compiled unmodified against this header instead of UPC++. There is one
// process and one rank: a collective returns its own argument, an rpc runs its callable at once, a future is
// ready when it is made. rank_n() is the one knob: the driver (oracle/ref_driver.cpp) sets it so that
// get_kmer_target_rank and the supermer cut of process_seq see a world of that size, while every update
// still lands in the one local table. Nothing here knows what a k-mer is.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <iomanip>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <string_view>
#include <type_traits>
#include <utility>

#define UPCXX_SERIALIZED_FIELDS(...)

namespace upcxx {

using intrank_t = int;

namespace standin {
inline intrank_t world_size = 1;  // what rank_n() and world().rank_n() report
}

inline intrank_t rank_me() { return 0; }
inline intrank_t rank_n() { return standin::world_size; }
inline void barrier() {}
inline void progress() {}

// No default constructor, so that `dist_object<T> d({})` can only mean a value-initialised T.
class team {
  bool is_world_;

 public:
  explicit team(bool is_world)
      : is_world_(is_world) {}
  intrank_t rank_me() const { return 0; }
  // the local team is this one process whatever the pretended world size
  intrank_t rank_n() const { return is_world_ ? standin::world_size : 1; }
};

inline team &world() {
  static team t(true);
  return t;
}

inline team &local_team() {
  static team t(false);
  return t;
}

template <typename T = void>
class future;

namespace standin {
template <typename R>
struct make_ready {
  template <typename F, typename... A>
  static future<R> call(F &&f, A &&...a);
};
template <>
struct make_ready<void> {
  template <typename F, typename... A>
  static future<void> call(F &&f, A &&...a);
};
template <typename R>
struct unwrap {
  using type = R;
};
template <typename R>
struct unwrap<future<R>> {
  using type = R;
};
}  // namespace standin

template <typename T>
class future {
  T value_{};

 public:
  future() = default;
  future(T v)
      : value_(std::move(v)) {}
  T wait() const { return value_; }
  T result() const { return value_; }
  bool ready() const { return true; }
  template <typename F>
  auto then(F &&f) const {
    using R = typename standin::unwrap<std::invoke_result_t<F, T>>::type;
    return standin::make_ready<R>::call(std::forward<F>(f), value_);
  }
};

template <>
class future<void> {
 public:
  void wait() const {}
  bool ready() const { return true; }
  template <typename F>
  auto then(F &&f) const {
    using R = typename standin::unwrap<std::invoke_result_t<F>>::type;
    return standin::make_ready<R>::call(std::forward<F>(f));
  }
};

namespace standin {
template <typename R>
template <typename F, typename... A>
future<R> make_ready<R>::call(F &&f, A &&...a) {
  return future<R>(f(std::forward<A>(a)...));
}
template <typename F, typename... A>
future<void> make_ready<void>::call(F &&f, A &&...a) {
  f(std::forward<A>(a)...);
  return future<void>();
}
}  // namespace standin

inline future<> make_future() { return future<>(); }
template <typename T>
future<T> make_future(T v) {
  return future<T>(std::move(v));
}
template <typename... F>
future<> when_all(F &&...) {
  return future<>();
}

template <typename T = void>
class promise {
  T value_{};

 public:
  void fulfill_result(T v) { value_ = std::move(v); }
  future<T> get_future() const { return future<T>(value_); }
  future<T> finalize() const { return future<T>(value_); }
};
template <>
class promise<void> {
 public:
  void fulfill_anonymous(std::intptr_t) {}
  void require_anonymous(std::intptr_t) {}
  future<> get_future() const { return future<>(); }
  future<> finalize() const { return future<>(); }
};

// Reductions over one rank: the result is the argument.
struct op_fast_add_t {};
struct op_fast_max_t {};
struct op_fast_min_t {};
inline constexpr op_fast_add_t op_fast_add{};
inline constexpr op_fast_max_t op_fast_max{};
inline constexpr op_fast_min_t op_fast_min{};

template <typename T, typename Op>
future<T> reduce_one(T v, Op, intrank_t, const team & = world()) {
  return future<T>(std::move(v));
}
template <typename T, typename Op>
future<T> reduce_all(T v, Op, const team & = world()) {
  return future<T>(std::move(v));
}

template <typename T>
class global_ptr {
  T *p_ = nullptr;

 public:
  global_ptr() = default;
  global_ptr(std::nullptr_t) {}
  explicit global_ptr(T *p)
      : p_(p) {}
  T *local() const { return p_; }
  bool is_null() const { return p_ == nullptr; }
  explicit operator bool() const { return p_ != nullptr; }
  bool operator==(const global_ptr &o) const { return p_ == o.p_; }
  bool operator!=(const global_ptr &o) const { return p_ != o.p_; }
};

template <typename T>
class dist_object {
  T value_;

 public:
  dist_object(T v, const team & = world())
      : value_(std::move(v)) {}
  template <typename... A>
  explicit dist_object(const team &, A &&...a)
      : value_(std::forward<A>(a)...) {}
  dist_object(const dist_object &) = delete;
  dist_object &operator=(const dist_object &) = delete;
  T *operator->() { return &value_; }
  const T *operator->() const { return &value_; }
  T &operator*() { return value_; }
  const T &operator*() const { return value_; }
};

// The one rank is the target of every rpc: run the callable now, hand back a ready future.
template <typename F, typename... A>
auto rpc(intrank_t, F &&f, A &&...a) {
  using R = typename standin::unwrap<std::invoke_result_t<F, A...>>::type;
  return standin::make_ready<R>::call(std::forward<F>(f), std::forward<A>(a)...);
}
template <typename F, typename... A>
void rpc_ff(intrank_t, F &&f, A &&...a) {
  f(std::forward<A>(a)...);
}

}  // namespace upcxx

// One-rank stand-in for upcxx_utils/log.hpp (TEST INFRASTRUCTURE ONLY, oracle/Makefile `ref`).
//
// The log macros write nothing to the terminal. SLOG* lines are appended to a buffer the driver can read (that is
// how it learns the count behind the reference's "Number dropped" line), WARN and SWARN bump a counter, DIE throws.
#pragma once

#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

#include <upcxx/upcxx.hpp>

#define KNORM ""
#define KLGREEN ""
#define KLRED ""
#define KLBLUE ""

// kmer_dht.hpp names both without a namespace, and includes only the aggregating stores of upcxx_utils
using upcxx::dist_object;
using upcxx::global_ptr;

namespace upcxx_utils {

// the reference's sources use these unqualified after `using namespace upcxx_utils`
using namespace upcxx;
using std::ifstream;
using std::ofstream;
using std::ostringstream;
using std::stringstream;

namespace standin {
inline int64_t num_warnings = 0;
inline std::string log_text;

template <typename... A>
std::string cat(const A &...a) {
  std::ostringstream os;
  (void)(os << ... << a);
  return os.str();
}

template <typename... A>
void log_line(const A &...a) {
  if (log_text.size() < (1u << 20)) log_text += cat(a...);
}

template <typename... A>
void warn(const A &...a) {
  num_warnings++;
  log_line("WARNING: ", a..., "\n");
}

template <typename... A>
[[noreturn]] void die(const char *file, int line, const A &...a) {
  throw std::runtime_error(cat("DIE at ", file, ":", line, ": ", a...));
}
}  // namespace standin

inline double get_free_mem() { return (double)sysconf(_SC_AVPHYS_PAGES) * (double)sysconf(_SC_PAGESIZE); }

inline std::string get_size_str(int64_t sz) { return std::to_string(sz) + "B"; }

// "<num> (<percent>%)": the driver reads the leading number back out of the "Number dropped" line
inline std::string perc_str(int64_t num, int64_t tot) {
  std::ostringstream os;
  os << num << " (" << std::fixed << std::setprecision(2) << (tot ? 100.0 * num / tot : 0.0) << "%)";
  return os.str();
}

inline std::string get_basename(const std::string &fname) {
  auto i = fname.rfind('/');
  return i == std::string::npos ? fname : fname.substr(i + 1);
}

inline std::string remove_file_ext(const std::string &fname) {
  auto i = fname.rfind('.');
  return i == std::string::npos ? fname : fname.substr(0, i);
}

// one rank writes into the working directory: the name stays as it is
inline std::string get_rank_path(std::string &fname, int) { return fname; }

}  // namespace upcxx_utils

#define SLOG(...) ::upcxx_utils::standin::log_line(__VA_ARGS__)
#define SLOG_VERBOSE(...) ::upcxx_utils::standin::log_line(__VA_ARGS__)
#define SOUT(...) ::upcxx_utils::standin::log_line(__VA_ARGS__)
#define LOG(...) ::upcxx_utils::standin::log_line(__VA_ARGS__)
#define DBG(...) ((void)0)
#define DBG_VERBOSE(...) ((void)0)
#define WARN(...) ::upcxx_utils::standin::warn(__VA_ARGS__)
#define SWARN(...) ::upcxx_utils::standin::warn(__VA_ARGS__)
#define DIE(...) ::upcxx_utils::standin::die(__FILE__, __LINE__, __VA_ARGS__)

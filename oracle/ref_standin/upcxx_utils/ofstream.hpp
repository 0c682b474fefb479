// One-rank stand-in for upcxx_utils/ofstream.hpp (TEST INFRASTRUCTURE ONLY): the one rank's part is the whole file.
#pragma once

#include <fstream>
#include <string>

#include "upcxx_utils/log.hpp"

namespace upcxx_utils {

class dist_ofstream : public std::ofstream {
 public:
  explicit dist_ofstream(const std::string &fname, bool append = false)
      : std::ofstream(fname, append ? std::ios::app : std::ios::trunc) {}
  int64_t get_last_known_tellp() { return (int64_t)tellp(); }
};

}  // namespace upcxx_utils

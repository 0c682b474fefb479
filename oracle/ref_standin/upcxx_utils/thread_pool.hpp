// One-rank stand-in for upcxx_utils/thread_pool.hpp (TEST INFRASTRUCTURE ONLY): the kcount path starts no threads.
#pragma once

#include "upcxx_utils/log.hpp"

// One-rank stand-in for upcxx_utils/mem_profile.hpp (TEST INFRASTRUCTURE ONLY): memory is not profiled.
#pragma once

#include "upcxx_utils/log.hpp"

#define LOG_MEM(...) ((void)0)

/* Stand-in for libkev's utils.h (the libkev submodule of the reference is
 * empty).  TEST INFRASTRUCTURE ONLY, written from scratch: what WSHandler.cpp
 * takes from it is the FALLTHROUGH marker between decodeFrame's switch cases
 * and, transitively, memcpy/memset and the fixed-width integer types. */
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__GNUC__) && __GNUC__ >= 7
#define FALLTHROUGH __attribute__((fallthrough))
#else
#define FALLTHROUGH ((void)0)
#endif

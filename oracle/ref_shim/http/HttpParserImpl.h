/* Stand-in for the reference's src/http/HttpParserImpl.h.  TEST
 * INFRASTRUCTURE ONLY, written from scratch.  WSHandler.h includes the real
 * header and uses nothing it declares; the real one drags in the HTTP parser
 * and more of the absent libkev.  What WSHandler.h does rely on arriving
 * through it: std::function, KMError (kmdefs.h) and KMBuffer (kmbuffer.h).
 * This directory stands before the reference's src/ on the include path. */
#pragma once

#include <functional>

#include "kmdefs.h"
#include "kmbuffer.h"

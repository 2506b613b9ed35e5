/* Stand-in for libkev's kmtrace.h (the libkev submodule of the reference is
 * empty).  TEST INFRASTRUCTURE ONLY, written from scratch: WSHandler.cpp
 * includes this header and traces nothing, so the trace macros are given as
 * no-ops in case a later revision of it does. */
#pragma once

#define KM_INFOTRACE(x) do { } while (0)
#define KM_WARNTRACE(x) do { } while (0)
#define KM_ERRTRACE(x) do { } while (0)
#define KM_DBGTRACE(x) do { } while (0)
#define KM_INFOXTRACE(x) do { } while (0)
#define KM_WARNXTRACE(x) do { } while (0)
#define KM_ERRXTRACE(x) do { } while (0)
#define KM_INFOTRACE_THIS(x) do { } while (0)
#define KM_WARNTRACE_THIS(x) do { } while (0)
#define KM_ERRTRACE_THIS(x) do { } while (0)

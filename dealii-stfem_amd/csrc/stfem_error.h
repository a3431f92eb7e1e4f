// The library's one error record: a thread-local text of at most 255 characters, read through stfem_last_error and its seven
// older synonyms (include/stfem.h), all defined in stfem_error.cpp.  Plain host C++; the HIP-side helpers on top of it are in
// stfem_hip_check.h.  Not part of the boundary.
#pragma once

#pragma GCC visibility push(hidden)
// Formats the reason of a failure into the calling thread's record (truncated to 255 characters) and returns `status`, so that
// a failing path reads `return stfem_set_error(STFEM_ERR_HIP, "...", ...)`.  The current text may be among the arguments.
int stfem_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#pragma GCC visibility pop

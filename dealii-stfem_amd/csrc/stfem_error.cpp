#include "stfem_error.h"

#include "../../include/stfem.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

static thread_local char g_error[256] = "";

int stfem_set_error(int status, const char *fmt, ...)
{
  char text[sizeof(g_error)]; // formatted aside: g_error itself may be one of the arguments
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof(text), fmt, ap);
  va_end(ap);
  memcpy(g_error, text, strlen(text) + 1);
  return status;
}

extern "C" {
const char *stfem_last_error(void) { return g_error; }
const char *stfem_last_hip_error(void) { return g_error; }
const char *stfem_comm_last_error(void) { return g_error; }
const char *stfem_transfer_last_error(void) { return g_error; }
const char *stfem_vanka_last_error(void) { return g_error; }
const char *stfem_driver_last_error(void) { return g_error; }
const char *stfem_stokes_last_hip_error(void) { return g_error; }
const char *stfem_stokes_vanka_last_error(void) { return g_error; }
}

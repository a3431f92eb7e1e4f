// CPU self-test of the library's error record (stfem_error.h / stfem_error.cpp): exit status 0 = all checks hold.
// Built by `make test_error` (host compiler only), run by tests/test_error_cpu.py.
#include "stfem_error.h"

#include "../../include/stfem.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++failures;                                \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
    }                                            \
  } while (0)

int main()
{
  CHECK(strcmp(stfem_last_error(), "") == 0, "a fresh thread has the text '%s'", stfem_last_error());

  // the format and the returned status
  int rc = stfem_set_error(STFEM_ERR_HIP, "%s: %s (%d of %zu)", "hipMalloc", "out of memory", 3, size_t(7));
  CHECK(rc == STFEM_ERR_HIP, "returned %d", rc);
  CHECK(strcmp(stfem_last_error(), "hipMalloc: out of memory (3 of 7)") == 0, "'%s'", stfem_last_error());
  rc = stfem_set_error(STFEM_ERR_COMM, "plain");
  CHECK(rc == STFEM_ERR_COMM && strcmp(stfem_last_error(), "plain") == 0, "%d '%s'", rc, stfem_last_error());

  // all eight accessors: the same record
  const char *(*const accessors[8])(void) = {stfem_last_error,         stfem_last_hip_error,   stfem_comm_last_error,
                                             stfem_transfer_last_error, stfem_vanka_last_error, stfem_driver_last_error,
                                             stfem_stokes_last_hip_error, stfem_stokes_vanka_last_error};
  for (int i = 0; i < 8; ++i) CHECK(accessors[i]() == stfem_last_error(), "accessor %d returns another pointer", i);

  // a message built from the current text itself
  stfem_set_error(STFEM_ERR_HIP, "inner %d", 42);
  rc = stfem_set_error(STFEM_ERR_UNSUPPORTED, "outer: (%s)", stfem_last_error());
  CHECK(rc == STFEM_ERR_UNSUPPORTED && strcmp(stfem_last_error(), "outer: (inner 42)") == 0, "%d '%s'", rc, stfem_last_error());

  // a second thread sees an empty record and does not disturb the first
  std::string seen_before = "?", seen_after = "?";
  const char *other = nullptr;
  std::thread([&] {
    seen_before = stfem_last_error();
    stfem_set_error(STFEM_ERR_HIP, "from the second thread");
    seen_after = stfem_last_error();
    other = stfem_last_error();
  }).join();
  CHECK(seen_before.empty(), "the second thread started with '%s'", seen_before.c_str());
  CHECK(seen_after == "from the second thread", "the second thread read '%s'", seen_after.c_str());
  CHECK(other != stfem_last_error(), "both threads share one record");
  CHECK(strcmp(stfem_last_error(), "outer: (inner 42)") == 0, "the first thread now reads '%s'", stfem_last_error());

  // 1000 characters: the first 255 and the terminator; the same with the long text as an argument of itself
  const std::string big(1000, 'x');
  rc = stfem_set_error(STFEM_ERR_HIP, "%s", big.c_str());
  CHECK(rc == STFEM_ERR_HIP && strlen(stfem_last_error()) == 255, "%d, length %zu", rc, strlen(stfem_last_error()));
  CHECK(std::string(stfem_last_error()) == big.substr(0, 255), "'%s'", stfem_last_error());
  stfem_set_error(STFEM_ERR_HIP, "y%s", stfem_last_error());
  CHECK(std::string(stfem_last_error()) == "y" + big.substr(0, 254), "'%s'", stfem_last_error());

  if (failures) printf("%d check(s) failed\n", failures);
  else printf("error record: all checks hold\n");
  return failures ? 1 : 0;
}

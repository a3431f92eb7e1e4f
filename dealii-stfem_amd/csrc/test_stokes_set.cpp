// CPU self-test of stfem_stokes_set.h (the set of one launch of the Stokes operator, how the entry points put it together and the
// destinations of a K-weighted term): exit status 0 = all checks hold, every comparison exact.  Built by `make test_stokes_set` (host
// compiler only; HOSTFLAGS takes -fsanitize=address,undefined), run by tests/test_stokes_set_cpu.py.
#include "stfem_stokes_set.h"

#include <cstdio>
#include <vector>

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

// what the flush callable has seen
struct Seen {
  std::vector<StokesSet> sets;
  std::vector<const double *> lin0;
};
struct Record {
  Seen *seen;
  int status;
  int operator()(const StokesSet &set, const double *const *lin) const
  {
    seen->sets.push_back(set);
    seen->lin0.push_back(lin[0]);
    return status;
  }
};
using Builder = StokesSetBuilder<Record>;

static double U[16], P[16], B[4]; // addresses to tell apart, never read
static const double eps10 = 10 * std::numeric_limits<double>::epsilon();
static const double zero = 0.0, one = 1.0;

static void test_threshold()
{
  Seen seen;
  Builder b(Record{&seen, 0});
  b.add_source(&U[0], &P[0]);
  const double above = std::nextafter(eps10, 1.0), neg = -eps10, neg_above = -above;
  char wu = 0, wp = 0;
  CHECK(b.add_destination(&U[1], &P[1], &eps10, &neg, &eps10, &wu, &wp) == 0, "status");
  CHECK(b.set.nout == 0 && wu == 0 && wp == 0, "weights of exactly 10 eps: the pair is skipped, its flags untouched (nout %d)", b.set.nout);
  CHECK(b.add_destination(&U[1], &P[1], &above, &neg_above, &zero, &wu, &wp) == 0, "status");
  const StokesSet &s = b.set;
  CHECK(s.nout == 1 && s.wKu[0][0] == above && s.wKp[0][0] == neg_above && s.wM[0][0] == 0.0, "the next double above 10 eps counts");
  CHECK(s.out_u[0] == &U[1] && s.out_p[0] == &P[1] && wu == 1 && wp == 1, "both parts are written");
  CHECK(b.flush() == 0 && seen.sets.size() == 1 && b.set.nout == 0, "flush launches once and empties the set");
  CHECK(b.flush() == 0 && seen.sets.size() == 1, "flush of an empty set does not launch");
}

static void test_store_flags_and_parts()
{
  Seen seen;
  Builder b(Record{&seen, 0});
  b.add_source(&U[0], &P[0], &B[0]);
  char wu = 0, wp = 0;
  // mass only: the pressure part has all-zero weights - null pointer, its flag untouched
  b.add_destination(&U[1], &P[1], &zero, &zero, &one, &wu, &wp);
  // the same pair again: the velocity part has been written, the pressure part is written first here
  b.add_destination(&U[1], &P[1], &one, &one, &zero, &wu, &wp);
  // no flag pointers: accumulated into, never stored
  b.add_destination(&U[2], &P[2], &one, &one, &one, nullptr, nullptr);
  // the pressure part alone
  char wu3 = 0, wp3 = 0;
  b.add_destination(&U[3], &P[3], &zero, &one, &zero, &wu3, &wp3);
  const StokesSet &s = b.set;
  CHECK(s.nsrc == 1 && s.us[0] == &U[0] && s.ps[0] == &P[0], "the source");
  CHECK(s.nout == 4, "nout %d", s.nout);
  CHECK(s.out_u[0] == &U[1] && s.out_p[0] == nullptr && s.store_u[0] == 1 && s.store_p[0] == 0, "pair 0: velocity stored, no pressure part");
  CHECK(s.wKu[0][0] == 0.0 && s.wKp[0][0] == 0.0 && s.wM[0][0] == 1.0, "pair 0: weights");
  CHECK(s.out_u[1] == &U[1] && s.out_p[1] == &P[1] && s.store_u[1] == 0 && s.store_p[1] == 1, "pair 1: velocity added, pressure stored");
  CHECK(wu == 1 && wp == 1, "flags of pairs 0 and 1");
  CHECK(s.out_u[2] == &U[2] && s.out_p[2] == &P[2] && s.store_u[2] == 0 && s.store_p[2] == 0, "pair 2: no flags, both parts added");
  CHECK(s.out_u[3] == nullptr && s.out_p[3] == &P[3] && s.store_u[3] == 0 && s.store_p[3] == 1 && wu3 == 0 && wp3 == 1, "pair 3: pressure alone");
  CHECK(b.flush() == 0 && seen.sets.size() == 1 && seen.sets[0].nout == 4 && seen.lin0[0] == &B[0], "the launch sees the set and lin");
}

// n_sources sources: the callable fires on reaching `full` pairs, with the status it returns handed on
static void test_full(int n_sources, int full)
{
  Seen seen;
  Builder b(Record{&seen, 7});
  for (int s = 0; s < n_sources; ++s) b.add_source(&U[s], &P[s]);
  const double w[MAXSRC] = {0.0, 0.0, 0.0, 2.0}, *a = w + (MAXSRC - n_sources); // the last source alone has a weight
  for (int o = 0; o < full + 1; ++o) {
    const int rc = b.add_destination(&U[4 + o], &P[4 + o], a, a, a, nullptr, nullptr);
    const bool fires = o == full - 1;
    CHECK(rc == (fires ? 7 : 0), "%d sources, pair %d: status %d", n_sources, o, rc);
    CHECK(int(seen.sets.size()) == (o >= full - 1 ? 1 : 0), "%d sources, pair %d: %zu launches", n_sources, o, seen.sets.size());
    CHECK(b.set.nout == (o < full - 1 ? o + 1 : o - (full - 1)), "%d sources, pair %d: nout %d", n_sources, o, b.set.nout);
  }
  CHECK(seen.sets[0].nout == full && seen.sets[0].nsrc == n_sources, "the launch holds %d pairs", full);
  CHECK(seen.sets[0].out_u[full - 1] == &U[4 + full - 1] && seen.sets[0].wKu[n_sources - 1][full - 1] == 2.0, "its last pair");
  CHECK(b.set.out_u[0] == &U[4 + full], "the pair after the launch opens the next set");
}

static void test_k_destinations()
{
  StokesSet set;
  set.nsrc = 2;
  set.nout = 5;
  for (int o = 0; o < 5; ++o) set.out_u[o] = &U[o];
  set.wKu[0][0] = 1.5;                       // destination 0: first source
  set.wM[0][1] = 3.0;                        // 1: mass only - not listed
  set.wKu[1][2] = -2.5;                      // 2: second source
  set.wKu[0][3] = 4.0; set.out_u[3] = nullptr; // 3: a weight but no velocity part - not listed
  set.wKu[0][4] = 0.5; set.wKu[1][4] = 0.25; // 4: both
  set.wKu[0][5] = 9.0; set.out_u[5] = &U[5]; // behind nout - not read
  double *out_u[MAXOUT];
  double wKu[MAXSRC][MAXOUT];
  for (int o = 0; o < MAXOUT; ++o) { out_u[o] = &U[15]; for (int s = 0; s < MAXSRC; ++s) wKu[s][o] = -1.0; }
  const int n = stokes_k_destinations(set, out_u, wKu);
  CHECK(n == 3, "%d destinations", n);
  CHECK(out_u[0] == &U[0] && out_u[1] == &U[2] && out_u[2] == &U[4], "the list, in the order of the set");
  CHECK(wKu[0][0] == 1.5 && wKu[1][0] == 0.0 && wKu[0][1] == 0.0 && wKu[1][1] == -2.5 && wKu[0][2] == 0.5 && wKu[1][2] == 0.25, "their weights");
  for (int o = 3; o < MAXOUT; ++o) CHECK(out_u[o] == nullptr, "slot %d behind the list is null", o);
  for (int o = 0; o < MAXOUT; ++o)
    for (int s = 0; s < MAXSRC; ++s) CHECK((o < 3 && s < 2) || wKu[s][o] == 0.0, "weight [%d][%d] outside the list is zero", s, o);
  const StokesSet single = stokes_single_set(&U[0], &U[1]);
  CHECK(stokes_k_destinations(single, out_u, wKu) == 1 && out_u[0] == &U[1] && wKu[0][0] == 1.0 && single.ps[0] == nullptr && single.out_p[0] == nullptr,
        "the one-source set");
}

int main()
{
  test_threshold();
  test_store_flags_and_parts();
  test_full(1, MAXOUT);
  test_full(2, MAXSRC);
  test_full(MAXSRC, MAXSRC);
  test_k_destinations();
  if (failures) printf("%d checks failed\n", failures);
  else printf("stfem_stokes_set.h: all checks hold\n");
  return failures ? 1 : 0;
}

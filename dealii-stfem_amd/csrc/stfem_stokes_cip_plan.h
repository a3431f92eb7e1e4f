// The grid of one CIP colour launch (stfem_stokes_cip.hip) and what stfem_stokes_last_cip_plan reports of it.  Host only, no HIP:
// test_stokes_cip_plan.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cstdlib>

struct CipPlan {
  long long grid;   // workgroups of the launch, >= 1
  long long passes; // rounds of the kernel's grid-stride loop: the longest run of cells of one cell slot
};

// n >= 1 cells of one colour, `slots` cells per workgroup at a time (degree 2: the 8 half-waves of a workgroup, limit 8 n_cu;
// degree 3: 1, the one wave of a workgroup, limit 32 n_cu), at most `limit` workgroups (what the device keeps busy), and at most `cap`
// when cap > 0 (STFEM_STOKES_CIP_WORKGROUPS).  Every cell is reached:
// grid * slots * passes >= n, and passes is the smallest such number.
inline CipPlan cip_plan(long long n, int slots, long long limit, long long cap)
{
  long long grid = std::min((n + slots - 1) / slots, std::max(1ll, limit));
  if (cap > 0) grid = std::min(grid, cap);
  grid = std::max(1ll, grid);
  return {grid, (n + grid * slots - 1) / (grid * slots)};
}

// STFEM_STOKES_CIP_WORKGROUPS as a cap: a positive whole number; unset, unparsable or non-positive: 0, no cap (a typo must not
// serialise the launches)
inline long long cip_parse_cap(const char *text)
{
  if (!text || !*text) return 0;
  char *end = nullptr;
  const long long v = std::strtoll(text, &end, 10);
  return (end == text || *end != '\0' || v < 1) ? 0 : v;
}

// The cells of a colour (bit d of colour: the parity of the cell index in direction d) of a mesh of nc cells
inline long long cip_colour_cells(const int nc[3], int colour)
{
  return (long long)((nc[0] - (colour & 1) + 1) / 2) * ((nc[1] - ((colour >> 1) & 1) + 1) / 2) * ((nc[2] - (colour >> 2) + 1) / 2);
}

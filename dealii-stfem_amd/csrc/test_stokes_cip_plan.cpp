// CPU self-test of the grid of a CIP colour launch (stfem_stokes_cip_plan.h): every cell is reached, the passes are the fewest that
// reach them, the cap and the limit hold, and without a cap the grid is the one the degree-2 launches always had.  Exit status 0.
#include "stfem_stokes_cip_plan.h"

#include <cstdio>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

int main()
{
  // what the launches pass: degree 3 one cell per workgroup under 32 n_cu, degree 2 eight under 8 n_cu (n_cu = 256, and a small device)
  const int slot_of[2] = {1, 8};
  const long long per_cu[2] = {32, 8};
  for (int k = 0; k < 2; ++k)
    for (long long n_cu : {1ll, 3ll, 256ll})
      for (long long cap : {0ll, 1ll, 2ll, 5000ll})
        for (long long n = 1; n <= 300; ++n) {
          const int slots = slot_of[k];
          const long long limit = per_cu[k] * n_cu;
          const CipPlan p = cip_plan(n, slots, limit, cap);
          CHECK(p.grid >= 1 && p.grid <= limit && (cap == 0 || p.grid <= cap));
          CHECK(p.passes >= 1 && p.grid * slots * p.passes >= n);          // every cell is reached
          CHECK(p.grid * slots * (p.passes - 1) < n);                      // in the fewest passes
          CHECK((p.grid - 1) * slots < n);                                 // no workgroup without a cell
          if (cap == 0) CHECK(p.grid == std::min((n + slots - 1) / slots, limit)); // the uncapped grid the degree-2 launches always had
        }
  // the cases of the GPU tests: 3 x 2 x 4 cells, colour 0 has 2 x 1 x 2 = 4 cells and colour 7 has 1 x 1 x 2: at degree 3 two
  // one-wave workgroups take the latter in one pass, capped at one workgroup it takes two passes; at degree 2 both cells sit in the
  // eight half-waves of one workgroup.  4 x 3 x 2 cells: colour 0 has 2 x 2 x 1.  A 48^3 mesh: 13824 cells per colour
  const int pert[3] = {3, 2, 4}, box[3] = {4, 3, 2}, big[3] = {48, 48, 48}, lone[3] = {1, 1, 1};
  long long total = 0;
  for (int colour = 0; colour < 8; ++colour) total += cip_colour_cells(pert, colour);
  CHECK(total == 24);
  CHECK(cip_colour_cells(pert, 0) == 4 && cip_colour_cells(pert, 7) == 1 * 1 * 2 && cip_colour_cells(box, 0) == 4);
  CHECK(cip_colour_cells(lone, 0) == 1 && cip_colour_cells(lone, 1) == 0 && cip_colour_cells(lone, 7) == 0);
  CHECK(cip_colour_cells(big, 5) == 13824);
  const long long last = cip_colour_cells(pert, 7);
  const CipPlan q3_free = cip_plan(last, 1, 32 * 256, 0), q3_capped = cip_plan(last, 1, 32 * 256, 1), q2_capped = cip_plan(last, 8, 8 * 256, 1);
  CHECK(q3_free.grid == 2 && q3_free.passes == 1 && q3_capped.grid == 1 && q3_capped.passes == 2);
  CHECK(q2_capped.grid == 1 && q2_capped.passes == 1);
  const CipPlan q3_wide = cip_plan(13824, 1, 32 * 256, 0), q2_wide = cip_plan(13824, 8, 8 * 256, 0); // the plans of profiles/stokes_q3_cip.txt
  CHECK(q3_wide.grid == 8192 && q3_wide.passes == 2 && q2_wide.grid == 1728 && q2_wide.passes == 1);
  // a non-positive limit still launches one workgroup
  CHECK(cip_plan(5, 1, 0, 0).grid == 1 && cip_plan(5, 1, 0, 0).passes == 5 && cip_plan(5, 8, -3, 0).passes == 1);
  // the cap of the environment: a positive number, anything else is no cap
  CHECK(cip_parse_cap(nullptr) == 0 && cip_parse_cap("") == 0 && cip_parse_cap("abc") == 0 && cip_parse_cap("0") == 0 && cip_parse_cap("-4") == 0);
  CHECK(cip_parse_cap("1") == 1 && cip_parse_cap(" 12") == 12 && cip_parse_cap("7x") == 0 && cip_parse_cap("3 ") == 0);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("stfem_stokes_cip_plan: ok\n");
  return 0;
}

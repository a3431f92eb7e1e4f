// The entry points of include/stfem.h that need no device: the temporal matrices, the 1D rules, the 1D factors of the space
// transfers, the level schedule of the multigrid, the mesh and coefficient helpers (host_tables.h behind the C-ABI) and the
// named trace ranges.  (C linkage: through the declarations in the header.)
#include "../../include/stfem.h"

#include "host_tables.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace stfem;

// ---- named trace ranges (roctx): the reference's TimerOutput scopes "vmult" / "Tvmult" (operators.h:539, 564, 590), "vanka"
// (stmg.h:835), "gmg" (stmg.h:1335, 1352) show up under the same names in `rocprofv3 --marker-trace`.  The roctx library of
// the profiler SDK is bound at run time; without it the calls do nothing.
namespace {
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
};
const Roctx &roctx()
{
  static Roctx r = [] {
    Roctx q;
    if (const char *e = getenv("STFEM_TRACE"))
      if (atoi(e) == 0) return q;
    void *h = nullptr;
    for (const char *n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
    }
    if (!h) return q;
    q.push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
    q.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!q.push || !q.pop) q.push = nullptr, q.pop = nullptr;
    return q;
  }();
  return r;
}

// time-multigrid transfer matrices (fe_time.h:749-898); out may be NULL to ask for the dimensions only
int time_transfer_out(int rc, const Mat &M, int m, int n, double *out, int32_t dims[2])
{
  if (rc != 0 || !dims) return STFEM_ERR_INVALID_ARGUMENT;
  dims[0] = m;
  dims[1] = n;
  if (out) std::copy(M.begin(), M.end(), out);
  return STFEM_OK;
}
} // namespace

void stfem_trace_push(const char *name)
{
  if (roctx().push) (void)roctx().push(name ? name : "stfem");
}
void stfem_trace_pop(void)
{
  if (roctx().pop) (void)roctx().pop();
}

int stfem_time_prolongation_matrix(int type, int r, int n_timesteps_at_once, double *out, int32_t dims[2])
{
  Mat M;
  int m = 0, n = 0;
  const int rc = time_prolongation(type, r, n_timesteps_at_once, M, m, n);
  return time_transfer_out(rc, M, m, n, out, dims);
}
int stfem_time_restriction_matrix(int type, int r, int n_timesteps_at_once, double *out, int32_t dims[2])
{
  Mat M;
  int m = 0, n = 0;
  const int rc = time_restriction(type, r, n_timesteps_at_once, M, m, n);
  return time_transfer_out(rc, M, m, n, out, dims);
}
int stfem_time_projection_matrix(int type, int r_src, int r_dst, int n_timesteps_at_once, double *out, int32_t dims[2])
{
  Mat M;
  int m = 0, n = 0;
  const int rc = time_projection(type, r_src, r_dst, n_timesteps_at_once, M, m, n);
  return time_transfer_out(rc, M, m, n, out, dims);
}
int stfem_time_evaluation_matrix(int type, int r, int samples_per_interval, double *out, int32_t dims[2])
{
  Mat M;
  int m = 0, n = 0;
  const int rc = time_evaluation(type, r, samples_per_interval, M, m, n);
  return time_transfer_out(rc, M, m, n, out, dims);
}

int stfem_fe_time_weights(int type, int r, double tau, int ns, double *Alpha, double *Beta,
                          double *Gamma, double *Zeta)
{
  if ((type != 0 && type != 1) || ns < 1 || !Alpha || !Beta || !Gamma || !Zeta || r > 8)
    return STFEM_ERR_INVALID_ARGUMENT;
  try {
    Mat A, B, G, Z;
    const int nb = fe_time_weights(type, r, tau, ns, A, B, G, Z);
    std::copy(A.begin(), A.end(), Alpha);
    std::copy(B.begin(), B.end(), Beta);
    std::copy(G.begin(), G.end(), Gamma);
    std::copy(Z.begin(), Z.end(), Zeta);
    return nb;
  } catch (...) {
    return STFEM_ERR_INVALID_ARGUMENT;
  }
}

int stfem_fe_time_weights_wave(int type, int r, double tau, int ns, double *AL, double *BL,
                               double *uK, double *uM, double *vM)
{
  if ((type != 0 && type != 1) || ns < 1 || !AL || !BL || !uK || !uM || !vM || r > 8)
    return STFEM_ERR_INVALID_ARGUMENT;
  try {
    Mat a, b, k, m, v;
    const int nb = fe_time_weights_wave(type, r, tau, ns, a, b, k, m, v);
    std::copy(a.begin(), a.end(), AL);
    std::copy(b.begin(), b.end(), BL);
    std::copy(k.begin(), k.end(), uK);
    std::copy(m.begin(), m.end(), uM);
    std::copy(v.begin(), v.end(), vM);
    return nb;
  } catch (...) {
    return STFEM_ERR_INVALID_ARGUMENT;
  }
}

int stfem_gauss_rule(int n, double *points, double *weights)
{
  if (n < 1 || n > 16 || !points || !weights) return STFEM_ERR_INVALID_ARGUMENT;
  std::vector<double> x, w;
  gauss_rule(n, x, w);
  std::copy(x.begin(), x.end(), points);
  std::copy(w.begin(), w.end(), weights);
  return STFEM_OK;
}

int stfem_fe_time_points(int type, int r, double *points)
{
  if ((type != 0 && type != 1) || r < 0 || r > 8 || !points) return STFEM_ERR_INVALID_ARGUMENT;
  // get_time_quad (fe_time.cc:152-161): QGaussLobatto(r + 1) for cG(r), QGaussRadau(r + 1, right) for dG(r)
  if (type == 0 && r < 1) return STFEM_ERR_INVALID_ARGUMENT;
  const std::vector<double> x = type == 0 ? lobatto_points(r + 1) : radau_right_points(r + 1);
  std::copy(x.begin(), x.end(), points);
  return STFEM_OK;
}

// ---- space-time multigrid: the 1D factors of a space transfer and the level schedule (fe_time.cc:17-150)
int stfem_transfer_line_matrices(int ncell_fine, int degree_fine, int ncell_coarse, int degree_coarse, double *P, double *I)
{
  if (ncell_coarse < 1 || degree_coarse < 1 || degree_fine < degree_coarse || (ncell_fine != ncell_coarse && ncell_fine != 2 * ncell_coarse))
    return STFEM_ERR_INVALID_ARGUMENT;
  std::vector<double> p, i;
  line_matrices(ncell_fine, degree_fine, ncell_coarse, degree_coarse, p, i);
  if (P) std::copy(p.begin(), p.end(), P);
  if (I) std::copy(i.begin(), i.end(), I);
  return STFEM_OK;
}

int stfem_poly_mg_sequence(int k_max, int k_min, int sequence_type, int32_t *out, int32_t *n_out)
{
  if (!n_out || k_min < 0 || k_max < k_min) return STFEM_ERR_INVALID_ARGUMENT;
  const std::vector<int> s = poly_mg_sequence(k_max, k_min, sequence_type);
  if (s.empty()) return STFEM_ERR_INVALID_ARGUMENT;
  if (out) std::copy(s.begin(), s.end(), out);
  *n_out = int32_t(s.size());
  return STFEM_OK;
}

int stfem_mg_sequence(int n_sp_lvl, int n_k, int n_p, int n_timesteps_at_once, int n_timesteps_at_once_min, char lower_lvl, int coarsening_type,
                      int time_before_space, int use_p_multigrid_space, int zip_from_back, char *out, int32_t *n_out)
{
  if (!n_out || n_sp_lvl < 1 || n_k < 1 || (use_p_multigrid_space && n_p < 1) || n_timesteps_at_once < 1 || n_timesteps_at_once_min < 1 ||
      (lower_lvl != 'k' && lower_lvl != 't'))
    return STFEM_ERR_INVALID_ARGUMENT;
  const std::string s = mg_sequence(n_sp_lvl, n_k, n_p, n_timesteps_at_once, n_timesteps_at_once_min, lower_lvl, coarsening_type,
                                    time_before_space != 0, use_p_multigrid_space != 0, zip_from_back != 0);
  if (out) std::copy(s.begin(), s.end(), out);
  *n_out = int32_t(s.size());
  return STFEM_OK;
}

int stfem_precondition_stmg_types(const char *mg_type_level, int n, int coarsening_type, int time_before_space, int smoother, int32_t *out)
{
  if (!mg_type_level || !out || n < 0) return STFEM_ERR_INVALID_ARGUMENT;
  const std::vector<int> r = precondition_stmg_types(std::string(mg_type_level, size_t(n)), coarsening_type, time_before_space != 0, smoother);
  std::copy(r.begin(), r.end(), out);
  return STFEM_OK;
}

int stfem_mesh_vertices(const int32_t gn[3], const double lo[3], const double up[3], double distort,
                        uint64_t seed, int32_t z0, int32_t z1, double *out)
{
  if (!gn || !lo || !up || !out || z0 < 0 || z1 > gn[2] || z0 >= z1) return STFEM_ERR_INVALID_ARGUMENT;
  mesh_vertices(gn, lo, up, distort, seed, z0, z1, out);
  return STFEM_OK;
}

int stfem_coefficient_per_cell(const int32_t nc[3], const double *vertices, double c1, double c2,
                               double c3, double distort, const int32_t sub[3], const double lo[3],
                               const double up[3], double *out)
{
  if (!nc || !vertices || !sub || !lo || !up || !out) return STFEM_ERR_INVALID_ARGUMENT;
  coefficient_per_cell(nc, vertices, c1, c2, c3, distort, sub, lo, up, out);
  return STFEM_OK;
}

// Precision traits of the operator's host side: the same launch logic (stfem_capi.hip) drives the fp64 (stfem::f64)
// and fp32 (stfem::f32) instantiations of the device code.  Included once per precision with STFEM_NS defined, like
// stfem_kernels_decl.h; no include guard on purpose.
#define STFEM_PREC_STR_(x) #x
#define STFEM_PREC_STR(x) STFEM_PREC_STR_(x)
namespace stfem {
namespace STFEM_NS {

struct Prec {
  using real = real_t;
  using Sweep = SweepParams;
  using Plan = TilePlan;
  using PPlan = PencilPlan;
  using Diag = DiagParams;
  static int atomic(int p, const Sweep &s, void *st) { return launch_cart_atomic(p, s, st); }
  static int geometry(int p, int nbm, int general, Plan &pl) { return tile_geometry(p, nbm, general, pl); }
  static int occupancy(int p, int nbm, int general)
  {
    static int cache[6][MAX_BLOCKS + 1][2] = {}; // 0 = not asked yet (one device type per process)
    int &v = cache[p][nbm][general];
    if (v == 0) v = std::max(1, tile_occupancy(p, nbm, general)) + 100;
    return v - 100;
  }
  static int tile(int p, const Sweep &s, const Plan &pl, void *st) { return launch_cart_tile(p, s, pl, st); }
  static int pencil_geometry(int p, int nbm, int ty, PPlan &pl) { return STFEM_NS::pencil_geometry(p, nbm, ty, pl); }
  static int pencil(int p, const Sweep &s, const PPlan &pl, void *st) { return launch_pencil(p, s, pl, st); }
  static int diagonal(const Diag &d, void *st) { return launch_diagonal(d, st); }
  static int metric(int p, const int nc[3], const double *v, const double *xq, const double *wq, const real *cl, int ll,
                    const real *cm, int ml, real *m, void *st)
  {
    return launch_build_metric(p, nc, v, xq, wq, cl, ll, cm, ml, m, st);
  }
  static const char *atomic_name() { return "st_sweep_cart_atomic<" STFEM_PREC_STR(STFEM_NS) ">"; }
  static const char *pencil_name() { return "st_sweep_pencil<" STFEM_PREC_STR(STFEM_NS) ">"; }
  static const char *tile_name(bool general)
  {
    return general ? "st_sweep_cart_tile<" STFEM_PREC_STR(STFEM_NS) ", stored metric>" : "st_sweep_cart_tile<" STFEM_PREC_STR(STFEM_NS) ">";
  }
};

} // namespace STFEM_NS
} // namespace stfem
#undef STFEM_PREC_STR
#undef STFEM_PREC_STR_

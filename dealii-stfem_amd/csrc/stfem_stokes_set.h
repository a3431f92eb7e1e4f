// One set of launches of the Stokes two-field operator: what varies from launch to launch - sources, destinations, weights, store
// flags - apart from the geometry and 1D tables of a context (stfem_stokes_internal.h), and how the entry points put one together.
// Plain C++, no device header: csrc/test_stokes_set.cpp checks it on the CPU.
#pragma once

#include <cmath>
#include <limits>

constexpr int MAXOUT = 8; // destination pairs of a launch with one source
constexpr int MAXSRC = 4; // sources, and destination pairs, of a launch with several sources

//   out_u[o] (=, +=) sum_s wKu[s][o] (nu K u_s - B^T p_s) + wM[s][o] M u_s,   out_p[o] (=, +=) sum_s wKp[s][o] B u_s
// It holds no geometry and does not depend on the velocity degree: stokes_params<DEG> writes it into the kernel argument of a degree.
struct StokesSet {
  // nsrc >= 1 sources (ps[s] == nullptr: u_s is read alone, mass only).  With several sources (SystemMatrixStokes::vmult with up to
  // MAXSRC source time dofs and up to MAXSRC destination pairs in ONE set of launches) a cell is evaluated for every source in turn,
  // the weighted results are summed in registers and scattered once; with one source the weights are applied at scatter time.
  int nsrc = 0;
  const double *us[MAXSRC] = {}, *ps[MAXSRC] = {};
  int nout = 0;
  double *out_u[MAXOUT] = {}, *out_p[MAXOUT] = {}; // (nullptr: this part of the pair is not written)
  double wKu[MAXSRC][MAXOUT] = {}, wKp[MAXSRC][MAXOUT] = {}, wM[MAXSRC][MAXOUT] = {}; // [source][destination pair]
  int store_u[MAXOUT] = {}, store_p[MAXOUT] = {}; // 1: the first cell to touch a DoF (lowest colour) stores, the others add; 0: all add
};

// One source, one velocity destination, weight 1 of the K part: a term applied by itself (CIP), a right-hand side (Nitsche data)
inline StokesSet stokes_single_set(const double *src_u, double *dst_u)
{
  StokesSet set;
  set.nsrc = set.nout = 1;
  set.us[0] = src_u; set.out_u[0] = dst_u; set.wKu[0][0] = 1.0;
  return set;
}

// The destinations that receive a K-weighted term on top of the linear operator (convection, CIP): those with a velocity part and a
// non-zero wKu for some source, in the order of the set, with their weights; the slots behind them are null / zero.  Returns their number.
inline int stokes_k_destinations(const StokesSet &set, double *out_u[MAXOUT], double wKu[MAXSRC][MAXOUT])
{
  for (int o = 0; o < MAXOUT; ++o) {
    out_u[o] = nullptr;
    for (int s = 0; s < MAXSRC; ++s) wKu[s][o] = 0.0;
  }
  int n = 0;
  for (int o = 0; o < set.nout; ++o) {
    bool use = false;
    for (int s = 0; s < set.nsrc; ++s) use = use || set.wKu[s][o] != 0.0;
    if (!use || !set.out_u[o]) continue;
    out_u[n] = set.out_u[o];
    for (int s = 0; s < set.nsrc; ++s) wKu[s][n] = set.wKu[s][o];
    ++n;
  }
  return n;
}

// A set in the making: the sources first, then the destination pairs with their weights per source.  flush(set, lin) launches it -
// lin[s]: the linearisation velocity of source s - and returns a status (0: ok).
template <class Flush> struct StokesSetBuilder {
  StokesSet set;
  const double *lin[MAXSRC] = {};
  Flush launch;
  explicit StokesSetBuilder(Flush flush) : launch(flush) {}
  void add_source(const double *u, const double *p, const double *b = nullptr) // (p == nullptr: mass only; b: linearisation velocity)
  {
    lin[set.nsrc] = b; set.us[set.nsrc] = u; set.ps[set.nsrc++] = p;
  }
  // The pair (u, p) receives  sum_s aU[s] (nu K u_s - B^T p_s) + bM[s] M u_s  and  sum_s aP[s] B u_s.  Weights up to 10 eps count
  // as zero (internal::scatter, operators.h:91-110); a part all of whose weights are zero is not touched (its pointer is null in the
  // launch), a pair of two such parts is left out.  written_u / written_p: whether an earlier launch has written that part - if
  // not, this one overwrites it and sets the flag; nullptr: the part is accumulated into.  Launches once the set is full.
  int add_destination(double *u, double *p, const double *aU, const double *aP, const double *bM, char *written_u, char *written_p)
  {
    const double eps10 = 10 * std::numeric_limits<double>::epsilon();
    const int o = set.nout;
    bool use_u = false, use_p = false;
    for (int s = 0; s < set.nsrc; ++s) {
      set.wKu[s][o] = std::abs(aU[s]) > eps10 ? aU[s] : 0.0;
      set.wKp[s][o] = std::abs(aP[s]) > eps10 ? aP[s] : 0.0;
      set.wM[s][o] = std::abs(bM[s]) > eps10 ? bM[s] : 0.0;
      use_u = use_u || set.wKu[s][o] != 0.0 || set.wM[s][o] != 0.0;
      use_p = use_p || set.wKp[s][o] != 0.0;
    }
    if (!use_u && !use_p) return 0;
    set.out_u[o] = use_u ? u : nullptr;
    set.out_p[o] = use_p ? p : nullptr;
    set.store_u[o] = use_u && written_u && !*written_u;
    set.store_p[o] = use_p && written_p && !*written_p;
    if (use_u && written_u) *written_u = 1;
    if (use_p && written_p) *written_p = 1;
    return ++set.nout == (set.nsrc > 1 ? MAXSRC : MAXOUT) ? flush() : 0;
  }
  int flush()
  {
    if (set.nout == 0) return 0;
    const int rc = launch(set, lin);
    set.nout = 0;
    return rc;
  }
};

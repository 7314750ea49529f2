// PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE / _ALL_SPARSE in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h:
// CartPlan::voldev_sparse) as a stand-alone host program under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by
// tests/test_split_route_sparse_plan_host.py.
//
// Over the product of tests/cpp/split_route_jacobian_plan_main.cpp -- model {0, 1, 3} x dimension {2, 3} x residual_only x phase
// {0, 1, 2} x scheme x material x layout x {whole box, sub-box} x {box, level lattice of the overlay} x forced chunk length, the
// split on and off -- with the routes {0 ... 15, 21, 23}:
//   - voldev_sparse is set exactly where voldev_jac is set, the route has bit 16 and the lattice is no level lattice: the full
//     assembly of a 3-D box under model 3 with the split on;
//   - in every other field the plan of route 21 / 23 is the plan of route 5 / 7;
//   - every plan of the routes 0 ... 15 equals, field by field, what the rule of the parent commit gives (parent_plan below:
//     that rule written out once more, independently of plan_cart), and has no voldev_sparse.
#include "pfm_cart_plan.h"

#include <cstdio>

using namespace pfm;

static int n_fail = 0;
#define CHECK(cond, ...)                                                                                                      \
  do                                                                                                                          \
    if (!(cond))                                                                                                              \
      {                                                                                                                       \
        ++n_fail;                                                                                                             \
        printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond);                                                             \
        printf(__VA_ARGS__);                                                                                                  \
        printf("\n");                                                                                                        \
      }                                                                                                                       \
  while (0)

static const int N_CU = 256;

static CartView box(int NX, int NY, int NZ, const int o0[3], const int o1[3])
{
  CartView cv{};
  cv.NX = NX, cv.NY = NY, cv.NZ = NZ;
  for (int d = 0; d < 3; ++d)
    cv.o0[d] = o0[d], cv.o1[d] = o1[d], cv.h[d] = 0.125;
  cv.owned_lex = 1;
  return cv;
}
static CartView whole(int ox, int oy, int oz)
{
  const int o0[3] = {0, 0, 0}, o1[3] = {ox - 1, oy - 1, oz - 1};
  return box(ox, oy, oz, o0, o1);
}
static CartView sub_box() // ghosts on every face, 13 planes
{
  const int o0[3] = {3, 2, 4}, o1[3] = {25, 20, 16};
  return box(30, 24, 20, o0, o1);
}

enum Scheme { STAGGERED, MONOLITHIC, PENALISED, KAPPA_LARGE, USE_OLD, N_SCHEMES };
static pfm_params params_of(int scheme, bool split)
{
  pfm_params p{};
  p.lambda = 1.0, p.mu = 1.0, p.constant_k = 1e-10, p.alpha_eps = 0.1, p.G_c = 1.0, p.alpha_biot = 0.0;
  p.timestep = 0.5, p.old_timestep = 0.5, p.old_old_timestep = 0.5, p.time = 2.0, p.timestep_number = 2;
  p.outer_solver = scheme == MONOLITHIC ? PFM_SOLVER_SIMPLE_MONOLITHIC : PFM_SOLVER_ACTIVE_SET;
  if (scheme == PENALISED || scheme == MONOLITHIC)
    p.gamma_penal = 10.0;
  if (scheme == KAPPA_LARGE)
    p.constant_k = 0.5;
  if (scheme == USE_OLD)
    p.use_old_timestep_pf = 1;
  if (split)
    p.decompose_stress_matrix = 1.0, p.decompose_stress_rhs = 0.5;
  return p;
}

// the rule of the parent commit: bits 1, 2, 4 and 8 of the route, no bit 16
static CartPlan parent_plan(const DevView &v, const CartView &cv, const pfm_params &p, int residual_only, int phase, const CartSplit &split)
{
  const Switches &sw = switches();
  const CartScheme sc = cart_scheme(p);
  CartPlan pl;
  pl.dim = v.dim, pl.phase = phase, pl.residual_only = residual_only != 0;
  const bool lattice_law = sc.split && v.dim == 3 && pl.residual_only;
  const int res_route = split.route & 3;
  pl.voldev = lattice_law && split.model == PFM_SPLIT_VOLDEV && (res_route == 1 || res_route == 3);
  pl.spectral = lattice_law && split.model == PFM_SPLIT_SPECTRAL && res_route == 3;
  pl.voldev_jac = sc.split && v.dim == 3 && !pl.residual_only && split.model == PFM_SPLIT_VOLDEV && (split.route & 4) != 0 && (split.route & 1) != 0 &&
                  (!cv.row_of_box || (split.route & 8) != 0);
  pl.supported = (!sc.split || pl.voldev || pl.spectral || pl.voldev_jac) && (v.dim == 2 || v.dim == 3);
  if (!pl.supported)
    return pl;
  pl.linear = sc.linear, pl.interleaved = v.layout == PFM_LAYOUT_INTERLEAVED, pl.het = cv.cell_lam != nullptr;
  pl.rows_residual = v.dim == 3 && !pl.residual_only && sc.linear && !sc.kappa_large && !sw.res_kernel && !pl.het && !pl.voldev_jac;
  pl.pair = pl.rows_residual && phase == 0 && !cv.row_of_box && !sw.jac_sequential && !sw.uu_clock && !sw.phi_clock;
  pl.one_launch = pl.cells2() && Switches::cart2d_one_launch();
  const bool whole_lex = cv.owned_lex && cv.o0[0] == 0 && cv.o0[1] == 0 && cv.o0[2] == 0 && cv.o1[0] == cv.NX - 1 && cv.o1[1] == cv.NY - 1 &&
                         cv.o1[2] == cv.NZ - 1 && phase == 0 && !cv.row_of_box && (long long)v.n_nodes == (long long)cv.NX * cv.NY * cv.NZ &&
                         v.n_owned == v.n_nodes && (long long)v.n_nodes * 32 < (1LL << 32) && !Switches::res_no_transfers();
  if (v.dim == 2 && pl.residual_only)
    pl.residual = PFM_RES_2M;
  else if (v.dim == 3 && !pl.rows_residual)
    pl.residual = (!(sc.linear && whole_lex) || pl.voldev || pl.spectral || pl.voldev_jac) ? PFM_RES_3
                  : (v.fused_solution && !pl.interleaved && v.n_nodes >= 64 && !Switches::res_no_wide_transfers()) ? PFM_RES_3X : PFM_RES_3D;
  pl.uu3_clock = sw.uu_clock && !pl.interleaved && !pl.het;
  pl.phi4_clock = (!pl.interleaved && !pl.het && sc.linear) ? sw.phi_clock : 0;
  const bool runs[PFM_TILE_KERNELS] = {pl.uu3() || pl.split3_jac(), pl.phi4(), pl.residual && v.dim == 3, pl.residual == PFM_RES_2M, pl.cells2()};
  for (int k = 0; k < PFM_TILE_KERNELS; ++k)
    if (runs[k])
      {
        CartView sel = cv;
        sel.tile_sel = pl.tile_sel(k);
        pl.grid[k] = cart_tile_grid(sel, k, N_CU);
      }
  return pl;
}

static bool same_grid(const TileGrid &a, const TileGrid &b)
{
  return a.ntx == b.ntx && a.nty == b.nty && a.zc == b.zc && a.nch == b.nch && a.n_tiles == b.n_tiles;
}
static bool same_plan(const CartPlan &a, const CartPlan &b)
{
  bool ok = a.dim == b.dim && a.phase == b.phase && a.residual_only == b.residual_only && a.supported == b.supported && a.voldev == b.voldev &&
            a.spectral == b.spectral && a.voldev_jac == b.voldev_jac && a.linear == b.linear && a.interleaved == b.interleaved && a.het == b.het &&
            a.rows_residual == b.rows_residual && a.pair == b.pair && a.residual == b.residual && a.one_launch == b.one_launch &&
            a.uu3_clock == b.uu3_clock && a.phi4_clock == b.phi4_clock && a.cells2() == b.cells2() && a.uu3() == b.uu3() && a.phi4() == b.phi4() &&
            a.split3_jac() == b.split3_jac();
  for (int k = 0; k < PFM_TILE_KERNELS; ++k)
    ok = ok && same_grid(a.grid[k], b.grid[k]) && a.tile_sel(k) == b.tile_sel(k);
  return ok;
}

int main()
{
  static const int32_t row_table[1] = {0};
  static const double lam[1] = {1.0};
  CHECK(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE == 21 && PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE == (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN | 16) &&
          PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE == 23 && PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE == (PFM_SPLIT_ROUTE_LATTICE_ALL | 16),
        "the route values");
  int n = 0, n_sparse = 0;
  for (int model : {PFM_SPLIT_REFERENCE, PFM_SPLIT_SPECTRAL, PFM_SPLIT_VOLDEV})
    for (int route : {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 21, 23})
      for (int dim : {2, 3})
        for (int ro : {0, 1})
          for (int phase : {0, 1, 2})
            for (int scheme = 0; scheme < N_SCHEMES; ++scheme)
              for (int het : {0, 1})
                for (int il : {0, 1})
                  for (int sub : {0, 1})
                    for (int level : {0, 1})
                      for (int forced : {0, 3})
                        for (int split : {0, 1})
                          {
                            CartView cv = dim == 2 ? whole(70, 9, 1) : sub ? sub_box() : whole(18, 17, 6);
                            cv.cell_lam = cv.cell_mu = het ? lam : nullptr;
                            cv.row_of_box = level ? row_table : nullptr;
                            cv.zc_force[PFM_ZC_UU3] = forced;
                            DevView v{};
                            v.dim = dim;
                            v.layout = il ? PFM_LAYOUT_INTERLEAVED : PFM_LAYOUT_BLOCKED;
                            v.n_nodes = cv.NX * cv.NY * cv.NZ;
                            v.n_owned = (cv.o1[0] - cv.o0[0] + 1) * (cv.o1[1] - cv.o0[1] + 1) * (cv.o1[2] - cv.o0[2] + 1);
                            const pfm_params p = params_of(scheme, split != 0);
                            const CartPlan pl = plan_cart(v, cv, p, ro, phase, N_CU, {model, route});
                            ++n;
                            if (!(route & 16))
                              {
                                CHECK(!pl.voldev_sparse && same_plan(pl, parent_plan(v, cv, p, ro, phase, {model, route})),
                                      "model %d route %d dim %d ro %d phase %d scheme %d het %d il %d sub %d level %d split %d differs from the parent's plan", model,
                                      route, dim, ro, phase, scheme, het, il, sub, level, split);
                                continue;
                              }
                            const CartPlan base = plan_cart(v, cv, p, ro, phase, N_CU, {model, route & ~16});
                            const bool want = split && model == PFM_SPLIT_VOLDEV && dim == 3 && !ro && !level;
                            n_sparse += want;
                            CHECK(pl.voldev_sparse == want && (!want || pl.voldev_jac) && pl.voldev_sparse == (base.voldev_jac && !level),
                                  "voldev_sparse %d: model %d route %d dim %d ro %d phase %d scheme %d het %d il %d sub %d level %d split %d", (int)pl.voldev_sparse,
                                  model, route, dim, ro, phase, scheme, het, il, sub, level, split);
                            CHECK(!base.voldev_sparse && same_plan(pl, base), "route %d is route %d in every other field (model %d dim %d ro %d phase %d level %d split %d)",
                                  route, route & ~16, model, dim, ro, phase, level, split);
                            if (want) // what the launch needs of the plan: the tiles and chunks of k_cart_uu3, whole, behind the residual kernel
                              CHECK(pl.split3_jac() == (phase != 1) && pl.tile_sel(PFM_ZC_UU3) == 0 && !pl.uu3() && !pl.phi4() && !pl.rows_residual && !pl.pair &&
                                      (phase == 1 || (pl.grid[PFM_ZC_UU3].n_tiles == (unsigned)(pl.grid[PFM_ZC_UU3].ntx * pl.grid[PFM_ZC_UU3].nty * pl.grid[PFM_ZC_UU3].nch) &&
                                                      pl.grid[PFM_ZC_UU3].n_tiles > 0)),
                                    "the sparse plan's Jacobian grid (route %d phase %d sub %d)", route, phase, sub);
                          }
  printf("split route sparse: %d plans, %d sparse\n", n, n_sparse);
  CHECK(n_sparse == 2 * 3 * N_SCHEMES * 2 * 2 * 2 * 2, "%d sparse plans", n_sparse);
  printf(n_fail ? "split_route_sparse_plan: %d FAILED\n" : "split_route_sparse_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

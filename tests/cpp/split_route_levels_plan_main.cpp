// PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS / _ALL_LEVELS (13, 15) in the plan of a cartesian assembly
// (cracks_amd/csrc/pfm_cart_plan.h: CartPlan::voldev_jac on a lattice with CartView::row_of_box) as a stand-alone host program
// under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by tests/test_split_route_levels_plan_host.py.
//
// Over model {0, 1, 3} x route {0, 1, 3, 5, 7, 13, 15} x dimension {2, 3} x residual_only x phase {0, 1, 2} x scheme x material x
// layout x {whole box, sub-box, level lattice of the overlay}, forced chunk lengths, the split on and off:
//   - every plan of routes 0, 1, 3, 5 and 7 equals, field by field, what the rule of the parent commit gives (parent_plan below:
//     that rule written out once more, independently of plan_cart);
//   - routes 13 and 15 are 5 and 7, field by field, everywhere but in the full model-3 split assembly of a level lattice;
//   - there: supported, voldev_jac, rows_residual == pair == false for every scheme, PFM_RES_3, k_cart_split3_jac over the tiles
//     and chunks of k_cart_uu3 ON THAT LEVEL'S LATTICE, neither k_cart_uu3 nor k_cart_phi4.
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

static CartView box(int NX, int NY, int NZ, const int o0[3], const int o1[3], int lex)
{
  CartView cv{};
  cv.NX = NX, cv.NY = NY, cv.NZ = NZ;
  for (int d = 0; d < 3; ++d)
    cv.o0[d] = o0[d], cv.o1[d] = o1[d], cv.h[d] = 0.125;
  cv.owned_lex = lex;
  return cv;
}
static CartView whole(int ox, int oy, int oz, int lex = 1)
{
  const int o0[3] = {0, 0, 0}, o1[3] = {ox - 1, oy - 1, oz - 1};
  return box(ox, oy, oz, o0, o1, lex);
}
static CartView sub_box() // ghosts on every face, 13 planes
{
  const int o0[3] = {3, 2, 4}, o1[3] = {25, 20, 16};
  return box(30, 24, 20, o0, o1, 1);
}
// a level lattice as finish_patches3d makes it: every node of the box may own a row (row_of_box says which), not lexicographic
static CartView level_lattice(const int32_t *rows)
{
  CartView cv = whole(15, 11, 15, 0);
  cv.row_of_box = rows;
  return cv;
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

// the rule of the parent commit: routes 0, 1, 3, 5 and 7; the Jacobian of the law on a box or sub-box only
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
                  !cv.row_of_box;
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
            a.split3_jac() == b.split3_jac() && a.oldf() == b.oldf() && a.residual_flag() == b.residual_flag();
  for (int k = 0; k < PFM_TILE_KERNELS; ++k)
    ok = ok && same_grid(a.grid[k], b.grid[k]) && a.tile_sel(k) == b.tile_sel(k);
  return ok;
}

int main()
{
  static const int32_t row_table[1] = {0};
  static const double lam[1] = {1.0};
  CHECK(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS == 13 && PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS == (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN | 8) &&
          PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS == 15 && PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS == (PFM_SPLIT_ROUTE_LATTICE_ALL | 8),
        "the route values");
  int n = 0, n_new = 0;
  for (int model : {PFM_SPLIT_REFERENCE, PFM_SPLIT_SPECTRAL, PFM_SPLIT_VOLDEV})
    for (int route : {0, 1, 3, 5, 7, 13, 15})
      for (int dim : {2, 3})
        for (int ro : {0, 1})
          for (int phase : {0, 1, 2})
            for (int scheme = 0; scheme < N_SCHEMES; ++scheme)
              for (int het : {0, 1})
                for (int il : {0, 1})
                  for (int where : {0, 1, 2}) // whole box, sub-box, level lattice
                    for (int forced : {0, 3})
                      for (int split : {0, 1})
                        {
                          const bool level = where == 2;
                          CartView cv = dim == 2 ? whole(70, 9, 1) : level ? level_lattice(row_table) : where == 1 ? sub_box() : whole(18, 17, 6);
                          if (dim == 2 && level)
                            cv.row_of_box = row_table; // (no such context exists; the plan must not care)
                          cv.cell_lam = cv.cell_mu = het ? lam : nullptr;
                          cv.zc_force[PFM_ZC_UU3] = forced;
                          DevView v{};
                          v.dim = dim;
                          v.layout = il ? PFM_LAYOUT_INTERLEAVED : PFM_LAYOUT_BLOCKED;
                          v.n_nodes = cv.NX * cv.NY * cv.NZ;
                          v.n_owned = (cv.o1[0] - cv.o0[0] + 1) * (cv.o1[1] - cv.o0[1] + 1) * (cv.o1[2] - cv.o0[2] + 1);
                          const pfm_params p = params_of(scheme, split != 0);
                          const CartPlan pl = plan_cart(v, cv, p, ro, phase, N_CU, {model, route});
                          ++n;
                          const bool is_new = (route & 8) && split && model == PFM_SPLIT_VOLDEV && dim == 3 && !ro && level;
                          if (!(route & 8))
                            CHECK(same_plan(pl, parent_plan(v, cv, p, ro, phase, {model, route})),
                                  "model %d route %d dim %d ro %d phase %d scheme %d het %d il %d where %d split %d differs from the parent's plan", model, route,
                                  dim, ro, phase, scheme, het, il, where, split);
                          else if (!is_new)
                            {
                              CHECK(same_plan(pl, plan_cart(v, cv, p, ro, phase, N_CU, {model, route & 7})) && same_plan(pl, parent_plan(v, cv, p, ro, phase, {model, route & 7})),
                                    "model %d route %d dim %d ro %d phase %d scheme %d het %d il %d where %d split %d: route %d is route %d here", model, route, dim,
                                    ro, phase, scheme, het, il, where, split, route, route & 7);
                              if (level)
                                CHECK(!pl.voldev_jac && !pl.split3_jac(), "no Jacobian of the law on this level");
                            }
                          if (!is_new)
                            continue;
                          ++n_new;
                          const CartPlan below = plan_cart(v, cv, p, ro, phase, N_CU, {model, route & 7});
                          CHECK(!below.supported && !below.voldev_jac, "routes 5 and 7 leave the level's full assembly to the general family");
                          CHECK(pl.supported && pl.voldev_jac && !pl.voldev && !pl.spectral && !pl.rows_residual && !pl.pair && pl.residual == PFM_RES_3 &&
                                  !pl.residual_only && !pl.cells2() && !pl.uu3() && !pl.phi4() && !pl.one_launch && pl.dim == 3 && pl.phase == phase,
                                "route %d phase %d scheme %d het %d il %d: supported %d voldev_jac %d rows %d pair %d residual %d", route, phase, scheme, het, il,
                                (int)pl.supported, (int)pl.voldev_jac, (int)pl.rows_residual, (int)pl.pair, (int)pl.residual);
                          CHECK(pl.interleaved == (il != 0) && pl.het == (het != 0) && pl.linear == cart_scheme(p).linear, "layout / material / scheme of the plan");
                          CHECK(pl.split3_jac() == (phase != 1), "k_cart_split3_jac runs whole (the overlay runs in phase 0 and 2 only)");
                          // the residual kernel: the grid of the level's residual-only plan under route 1
                          const CartPlan res = plan_cart(v, cv, p, 1, phase, N_CU, {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_LATTICE});
                          CHECK(res.voldev && same_grid(pl.grid[PFM_ZC_RES3], res.grid[PFM_ZC_RES3]) && pl.tile_sel(PFM_ZC_RES3) == phase &&
                                  pl.grid[PFM_ZC_RES3].n_tiles > 0,
                                "the residual kernel's grid and selection");
                          // the Jacobian kernel: every tile of k_cart_uu3's geometry over THIS lattice (15 x 11 x 15 nodes) with its chunk length
                          CartView all = cv;
                          all.tile_sel = 0;
                          const TileGrid want = cart_tile_grid(all, PFM_ZC_UU3, N_CU);
                          if (phase != 1)
                            CHECK(same_grid(pl.grid[PFM_ZC_UU3], want) && pl.tile_sel(PFM_ZC_UU3) == 0 && want.ntx == 2 && want.nty == 3 &&
                                    want.n_tiles == (unsigned)(2 * 3 * want.nch) && want.nch == (15 + want.zc - 1) / want.zc && (!forced || want.zc == forced),
                                  "the Jacobian kernel's grid: %d x %d x %d (zc %d)", pl.grid[PFM_ZC_UU3].ntx, pl.grid[PFM_ZC_UU3].nty, pl.grid[PFM_ZC_UU3].nch,
                                  pl.grid[PFM_ZC_UU3].zc);
                          else
                            CHECK(pl.grid[PFM_ZC_UU3].n_tiles == 0, "nothing of the Jacobian in phase 1");
                          CHECK(pl.grid[PFM_ZC_PHI4].n_tiles == 0 && pl.grid[PFM_ZC_RES2].n_tiles == 0 && pl.grid[PFM_TILES_CELLS2].n_tiles == 0, "no other kernel");
                        }
  printf("split route levels: %d plans, %d on the level kernels\n", n, n_new);
  CHECK(n_new == 2 * 3 * N_SCHEMES * 2 * 2 * 2, "%d new plans", n_new);
  printf(n_fail ? "split_route_levels_plan: %d FAILED\n" : "split_route_levels_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

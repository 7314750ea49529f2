// PFM_SPLIT_ROUTE_LATTICE_JACOBIAN / _ALL in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h: CartPlan::voldev_jac)
// as a stand-alone host program under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by
// tests/test_split_route_jacobian_plan_host.py.
//
// Over model {0, 1, 3} x route {0, 1, 3, 5, 7} x dimension {2, 3} x residual_only x phase {0, 1, 2} x scheme x material x layout x
// {whole box, sub-box} x {box, level lattice of the overlay}, the split on and off:
//   - the full assembly of a 3-D box (not a level lattice) under model 3 with the split on and bit 4 of the route is the one new
//     supported plan: voldev_jac, rows_residual == pair == false for every scheme, PFM_RES_3 cut into halves, k_cart_split3_jac
//     whole in phase 0 and 2 over the tiles and chunks of k_cart_uu3, neither k_cart_uu3 nor k_cart_phi4;
//   - the residual-only plans of routes 5 and 7 are those of routes 1 and 3, field by field;
//   - every plan of routes 0, 1 and 3 -- and of 5 and 7 where the new plan does not apply -- equals, field by field, what the
//     rule of the parent commit gives (parent_plan below: that rule written out once more, independently of plan_cart).
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

// the rule of the parent commit: routes 0, 1 and 3 only, no Jacobian kernel with a split form
static CartPlan parent_plan(const DevView &v, const CartView &cv, const pfm_params &p, int residual_only, int phase, const CartSplit &split)
{
  const Switches &sw = switches();
  const CartScheme sc = cart_scheme(p);
  CartPlan pl;
  pl.dim = v.dim, pl.phase = phase, pl.residual_only = residual_only != 0;
  const bool lattice_law = sc.split && v.dim == 3 && pl.residual_only;
  pl.voldev = lattice_law && split.model == PFM_SPLIT_VOLDEV && (split.route == 1 || split.route == 3);
  pl.spectral = lattice_law && split.model == PFM_SPLIT_SPECTRAL && split.route == 3;
  pl.supported = (!sc.split || pl.voldev || pl.spectral) && (v.dim == 2 || v.dim == 3);
  if (!pl.supported)
    return pl;
  pl.linear = sc.linear, pl.interleaved = v.layout == PFM_LAYOUT_INTERLEAVED, pl.het = cv.cell_lam != nullptr;
  pl.rows_residual = v.dim == 3 && !pl.residual_only && sc.linear && !sc.kappa_large && !sw.res_kernel && !pl.het;
  pl.pair = pl.rows_residual && phase == 0 && !cv.row_of_box && !sw.jac_sequential && !sw.uu_clock && !sw.phi_clock;
  pl.one_launch = pl.cells2() && Switches::cart2d_one_launch();
  const bool whole_lex = cv.owned_lex && cv.o0[0] == 0 && cv.o0[1] == 0 && cv.o0[2] == 0 && cv.o1[0] == cv.NX - 1 && cv.o1[1] == cv.NY - 1 &&
                         cv.o1[2] == cv.NZ - 1 && phase == 0 && !cv.row_of_box && (long long)v.n_nodes == (long long)cv.NX * cv.NY * cv.NZ &&
                         v.n_owned == v.n_nodes && (long long)v.n_nodes * 32 < (1LL << 32) && !Switches::res_no_transfers();
  if (v.dim == 2 && pl.residual_only)
    pl.residual = PFM_RES_2M;
  else if (v.dim == 3 && !pl.rows_residual)
    pl.residual = (!(sc.linear && whole_lex) || pl.voldev || pl.spectral) ? PFM_RES_3
                  : (v.fused_solution && !pl.interleaved && v.n_nodes >= 64 && !Switches::res_no_wide_transfers()) ? PFM_RES_3X : PFM_RES_3D;
  pl.uu3_clock = sw.uu_clock && !pl.interleaved && !pl.het;
  pl.phi4_clock = (!pl.interleaved && !pl.het && sc.linear) ? sw.phi_clock : 0;
  const bool runs[PFM_TILE_KERNELS] = {pl.uu3(), pl.phi4(), pl.residual && v.dim == 3, pl.residual == PFM_RES_2M, pl.cells2()};
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
  CHECK(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN == 5 && PFM_SPLIT_ROUTE_LATTICE_JACOBIAN == (PFM_SPLIT_ROUTE_LATTICE | 4) && PFM_SPLIT_ROUTE_LATTICE_ALL == 7 &&
          PFM_SPLIT_ROUTE_LATTICE_ALL == (PFM_SPLIT_ROUTE_LATTICE_ANY | 4),
        "the route values");
  int n = 0, n_new = 0;
  for (int model : {PFM_SPLIT_REFERENCE, PFM_SPLIT_SPECTRAL, PFM_SPLIT_VOLDEV})
    for (int route : {0, 1, 3, 5, 7})
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
                            const bool is_new = split && model == PFM_SPLIT_VOLDEV && (route & 4) && dim == 3 && !ro && !level;
                            if (!is_new)
                              {
                                // routes 5 and 7 act as 1 and 3 here; routes 0, 1, 3: the parent's rule
                                const CartPlan parent = parent_plan(v, cv, p, ro, phase, {model, route & 3});
                                CHECK(!pl.voldev_jac && !pl.split3_jac() && same_plan(pl, parent),
                                      "model %d route %d dim %d ro %d phase %d scheme %d het %d il %d sub %d level %d split %d differs from the parent's plan", model,
                                      route, dim, ro, phase, scheme, het, il, sub, level, split);
                                if (route & 4)
                                  CHECK(same_plan(pl, plan_cart(v, cv, p, ro, phase, N_CU, {model, route & 3})), "route %d is route %d here", route, route & 3);
                                continue;
                              }
                            ++n_new;
                            CHECK(pl.supported && pl.voldev_jac && !pl.voldev && !pl.spectral && !pl.rows_residual && !pl.pair && pl.residual == PFM_RES_3 &&
                                    !pl.residual_only && !pl.cells2() && !pl.uu3() && !pl.phi4() && !pl.one_launch && pl.dim == 3 && pl.phase == phase,
                                  "route %d phase %d scheme %d het %d il %d sub %d: supported %d voldev_jac %d rows %d pair %d residual %d", route, phase, scheme, het,
                                  il, sub, (int)pl.supported, (int)pl.voldev_jac, (int)pl.rows_residual, (int)pl.pair, (int)pl.residual);
                            CHECK(pl.interleaved == (il != 0) && pl.het == (het != 0) && pl.linear == cart_scheme(p).linear, "layout / material / scheme of the plan");
                            CHECK(pl.split3_jac() == (phase != 1), "k_cart_split3_jac runs whole, in phase 0 and in the second half");
                            // the residual kernel is the one cut into halves, with the grid of the residual-only plan of route 1
                            const CartPlan res = plan_cart(v, cv, p, 1, phase, N_CU, {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_LATTICE});
                            CHECK(res.voldev && same_grid(pl.grid[PFM_ZC_RES3], res.grid[PFM_ZC_RES3]) && pl.tile_sel(PFM_ZC_RES3) == phase &&
                                    pl.grid[PFM_ZC_RES3].n_tiles > 0,
                                  "the residual kernel's grid and selection");
                            // the Jacobian kernel: every tile (selection 0) of k_cart_uu3's geometry with its chunk length
                            CartView all = cv;
                            all.tile_sel = 0;
                            const TileGrid want = cart_tile_grid(all, PFM_ZC_UU3, N_CU);
                            if (phase != 1)
                              CHECK(same_grid(pl.grid[PFM_ZC_UU3], want) && pl.tile_sel(PFM_ZC_UU3) == 0 && want.n_tiles > 0 && (!forced || want.zc == forced),
                                    "the Jacobian kernel's grid: %d x %d x %d (zc %d)", pl.grid[PFM_ZC_UU3].ntx, pl.grid[PFM_ZC_UU3].nty, pl.grid[PFM_ZC_UU3].nch,
                                    pl.grid[PFM_ZC_UU3].zc);
                            else
                              CHECK(pl.grid[PFM_ZC_UU3].n_tiles == 0, "nothing of the Jacobian in phase 1");
                            CHECK(pl.grid[PFM_ZC_PHI4].n_tiles == 0 && pl.grid[PFM_ZC_RES2].n_tiles == 0 && pl.grid[PFM_TILES_CELLS2].n_tiles == 0, "no other kernel");
                          }
  printf("split route jacobian: %d plans, %d on the lattice kernels\n", n, n_new);
  CHECK(n_new == 2 * 3 * N_SCHEMES * 2 * 2 * 2 * 2, "%d new plans", n_new);
  printf(n_fail ? "split_route_jacobian_plan: %d FAILED\n" : "split_route_jacobian_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

// The split route in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h: CartSplit, CartPlan::voldev) as a
// stand-alone host program under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by tests/test_split_route_plan_host.py.
//
// Over dimension x phase x residual_only x scheme x material x layout x fused x level x {no split, split with the default route,
// split with the lattice route under model 3, the same under model 1}, on a whole box and on a partitioned one:
//   - the residual-only assembly of a 3-D lattice with the split on, model 3 and the lattice route is the ONE supported split
//     plan: PFM_RES_3 through CartPlan::voldev, never rows_residual, never the pair, no Jacobian kernel, and the tile grid and
//     the cut into halves of an unsplit PFM_RES_3 plan of the same lattice and phase;
//   - every other combination is, field by field, what plan_cart gives without the new argument.
#include "pfm_cart_plan.h"

#include <cstdio>
#include <cstring>

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
// a rank in the middle of a partition: ghosts on every face, 2 x 2 tiles of the residual kernel, 13 planes
static CartView sub_box()
{
  const int o0[3] = {3, 2, 4}, o1[3] = {25, 20, 16};
  return box(30, 24, 20, o0, o1);
}

enum Scheme { STAGGERED, MONOLITHIC, PENALISED, KAPPA_LARGE, N_SCHEMES };
static pfm_params params_of(int scheme, bool split)
{
  pfm_params p{};
  p.lambda = 1.0, p.mu = 1.0, p.constant_k = 1e-10, p.alpha_eps = 0.1, p.G_c = 1.0, p.alpha_biot = 0.0;
  p.timestep = 0.5, p.old_timestep = 0.5, p.old_old_timestep = 0.5, p.time = 2.0, p.timestep_number = 2;
  p.outer_solver = scheme == MONOLITHIC ? PFM_SOLVER_SIMPLE_MONOLITHIC : PFM_SOLVER_ACTIVE_SET;
  if (scheme == PENALISED)
    p.gamma_penal = 10.0;
  if (scheme == KAPPA_LARGE)
    p.constant_k = 0.5;
  if (split)
    p.decompose_stress_matrix = 1.0, p.decompose_stress_rhs = 1.0;
  return p;
}

static bool same_grid(const TileGrid &a, const TileGrid &b)
{
  return a.ntx == b.ntx && a.nty == b.nty && a.zc == b.zc && a.nch == b.nch && a.n_tiles == b.n_tiles;
}
static bool same_plan(const CartPlan &a, const CartPlan &b)
{
  bool ok = a.dim == b.dim && a.phase == b.phase && a.residual_only == b.residual_only && a.supported == b.supported && a.voldev == b.voldev &&
            a.linear == b.linear && a.interleaved == b.interleaved && a.het == b.het && a.rows_residual == b.rows_residual && a.pair == b.pair &&
            a.residual == b.residual && a.one_launch == b.one_launch && a.uu3_clock == b.uu3_clock && a.phi4_clock == b.phi4_clock &&
            a.cells2() == b.cells2() && a.uu3() == b.uu3() && a.phi4() == b.phi4();
  for (int k = 0; k < PFM_TILE_KERNELS; ++k)
    ok = ok && same_grid(a.grid[k], b.grid[k]) && a.tile_sel(k) == b.tile_sel(k);
  return ok;
}

int main()
{
  static const int32_t row_table[1] = {0}, bnd[3] = {0, 1, 2};
  static const double lam[1] = {1.0}, sol[1] = {0.0};
  const CartSplit arms[4] = {CartSplit(), {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_GENERAL}, {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_LATTICE},
                             {PFM_SPLIT_SPECTRAL, PFM_SPLIT_ROUTE_LATTICE}};
  CHECK(arms[0].model == PFM_SPLIT_REFERENCE && arms[0].route == PFM_SPLIT_ROUTE_GENERAL, "the default of CartSplit");
  int n = 0, n_new = 0;
  for (int dim : {2, 3})
    for (int phase : {0, 1, 2})
      for (int ro : {0, 1})
        for (int scheme = 0; scheme < N_SCHEMES; ++scheme)
          for (int het : {0, 1})
            for (int il : {0, 1})
              for (int sub : {0, 1})
                for (int fused : {0, 1})
                  for (int level : {0, 1})
                    for (int listed : {0, 1})
                      for (int forced : {0, 2})
                        for (int split : {0, 1})
                          for (int arm = 0; arm < 4; ++arm)
                            {
                              CartView cv = dim == 2 ? whole(70, 9, 1) : sub ? sub_box() : whole(18, 17, 6);
                              if (dim == 2 && sub)
                                cv.NX += 3, cv.o0[0] += 2, cv.o1[0] += 2;
                              cv.cell_lam = cv.cell_mu = het ? lam : nullptr;
                              cv.row_of_box = level ? row_table : nullptr;
                              cv.zc_force[PFM_ZC_RES3] = forced;
                              if (listed) // the boundary-tile list of the second half, for the chunk length of this lattice
                                {
                                  CartView c0 = cv;
                                  cv.bnd_res3 = bnd, cv.n_bnd_res3 = 3, cv.zc_res3 = cart_tile_grid(c0, PFM_ZC_RES3, N_CU).zc;
                                }
                              DevView v{};
                              v.dim = dim;
                              v.layout = il ? PFM_LAYOUT_INTERLEAVED : PFM_LAYOUT_BLOCKED;
                              v.n_nodes = cv.NX * cv.NY * cv.NZ;
                              v.n_owned = (cv.o1[0] - cv.o0[0] + 1) * (cv.o1[1] - cv.o0[1] + 1) * (cv.o1[2] - cv.o0[2] + 1);
                              v.fused_solution = fused ? sol : nullptr;
                              const pfm_params p = params_of(scheme, split != 0);
                              const CartPlan base = plan_cart(v, cv, p, ro, phase, N_CU); // today's answer
                              const CartPlan pl = plan_cart(v, cv, p, ro, phase, N_CU, arms[arm]);
                              ++n;
                              CHECK(!base.voldev && base.supported == !split, "the default: split %d supported %d", split, (int)base.supported);
                              const bool is_new = split && arm == 2 && dim == 3 && ro;
                              if (!is_new)
                                {
                                  CHECK(same_plan(pl, base), "dim %d phase %d ro %d scheme %d het %d il %d sub %d fused %d level %d split %d arm %d differs from the default",
                                        dim, phase, ro, scheme, het, il, sub, fused, level, split, arm);
                                  continue;
                                }
                              ++n_new;
                              CHECK(pl.supported && pl.voldev && pl.residual == PFM_RES_3 && !pl.rows_residual && !pl.pair && !pl.cells2() && !pl.uu3() && !pl.phi4() &&
                                      !pl.one_launch && pl.residual_only && pl.dim == 3 && pl.phase == phase,
                                    "phase %d scheme %d het %d il %d sub %d fused %d level %d: supported %d voldev %d residual %d rows %d pair %d", phase, scheme, het, il,
                                    sub, fused, level, (int)pl.supported, (int)pl.voldev, (int)pl.residual, (int)pl.rows_residual, (int)pl.pair);
                              CHECK(pl.interleaved == (il != 0) && pl.het == (het != 0), "layout / material of the split plan");
                              // the unsplit PFM_RES_3 plan of this lattice and phase: the penalised scheme has no polynomial form
                              const CartPlan un = plan_cart(v, cv, params_of(PENALISED, false), ro, phase, N_CU);
                              CHECK(un.supported && un.residual == PFM_RES_3 && !un.voldev, "the yardstick is an unsplit PFM_RES_3 plan");
                              for (int k = 0; k < PFM_TILE_KERNELS; ++k)
                                CHECK(same_grid(pl.grid[k], un.grid[k]) && pl.tile_sel(k) == un.tile_sel(k), "kernel %d: grid %d x %d x %d (zc %d, %u tiles) sel %d, unsplit %d x %d x %d (zc %d, %u tiles) sel %d",
                                      k, pl.grid[k].ntx, pl.grid[k].nty, pl.grid[k].nch, pl.grid[k].zc, pl.grid[k].n_tiles, pl.tile_sel(k), un.grid[k].ntx,
                                      un.grid[k].nty, un.grid[k].nch, un.grid[k].zc, un.grid[k].n_tiles, un.tile_sel(k));
                              CHECK(pl.grid[PFM_ZC_RES3].n_tiles > 0 && pl.tile_sel(PFM_ZC_RES3) == phase, "the residual kernel is the one cut into halves");
                              if (phase == 2 && listed)
                                CHECK(pl.grid[PFM_ZC_RES3].n_tiles == 3u, "the second half runs over the list: %u tiles", pl.grid[PFM_ZC_RES3].n_tiles);
                            }
  printf("split route: %d plans, %d on the lattice\n", n, n_new);
  CHECK(n_new == 3 * N_SCHEMES * 2 * 2 * 2 * 2 * 2 * 2 * 2, "%d new plans", n_new);
  printf(n_fail ? "split_route_plan: %d FAILED\n" : "split_route_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

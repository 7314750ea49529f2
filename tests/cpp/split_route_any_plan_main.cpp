// PFM_SPLIT_ROUTE_LATTICE_ANY in the plan of a cartesian assembly (cracks_amd/csrc/pfm_cart_plan.h: CartPlan::spectral next to
// CartPlan::voldev) as a stand-alone host program under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by
// tests/test_split_route_any_plan_host.py.
//
// Over the product of tests/cpp/split_route_plan_main.cpp (dimension x phase x residual_only x scheme x material x layout x
// partition x fused x level x listed x forced chunk x split), with the arms {model 1, route 3}, {model 3, route 3} and, as
// combinations that must change nothing, {model 1, route 0}, {model 0, route 3}, {model 1, route 1}:
//   - the spectral plan (the residual-only assembly of a 3-D lattice with the split on, model 1, route 3) equals, field by field
//     except spectral / voldev, the voldev plan (model 3, route 1) of the same lattice and phase;
//   - the model-3 route-3 plan equals the model-3 route-1 plan in every field;
//   - every other combination is, field by field, what plan_cart gives without the argument.
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
// every field and every answer of a plan but the two laws
static bool same_but_the_law(const CartPlan &a, const CartPlan &b)
{
  bool ok = a.dim == b.dim && a.phase == b.phase && a.residual_only == b.residual_only && a.supported == b.supported &&
            a.linear == b.linear && a.interleaved == b.interleaved && a.het == b.het && a.rows_residual == b.rows_residual && a.pair == b.pair &&
            a.residual == b.residual && a.one_launch == b.one_launch && a.uu3_clock == b.uu3_clock && a.phi4_clock == b.phi4_clock &&
            a.cells2() == b.cells2() && a.uu3() == b.uu3() && a.phi4() == b.phi4() && a.oldf() == b.oldf() && a.residual_flag() == b.residual_flag();
  for (int k = 0; k < PFM_TILE_KERNELS; ++k)
    ok = ok && same_grid(a.grid[k], b.grid[k]) && a.tile_sel(k) == b.tile_sel(k);
  return ok;
}
static bool same_plan(const CartPlan &a, const CartPlan &b) { return same_but_the_law(a, b) && a.voldev == b.voldev && a.spectral == b.spectral; }

int main()
{
  static const int32_t row_table[1] = {0}, bnd[3] = {0, 1, 2};
  static const double lam[1] = {1.0}, sol[1] = {0.0};
  enum { DEFAULT, SPECTRAL_ANY, VOLDEV_ANY, SPECTRAL_GENERAL, REFERENCE_ANY, SPECTRAL_LATTICE, N_ARMS };
  const CartSplit arms[N_ARMS] = {CartSplit(),
                                  {PFM_SPLIT_SPECTRAL, PFM_SPLIT_ROUTE_LATTICE_ANY},
                                  {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_LATTICE_ANY},
                                  {PFM_SPLIT_SPECTRAL, PFM_SPLIT_ROUTE_GENERAL},
                                  {PFM_SPLIT_REFERENCE, PFM_SPLIT_ROUTE_LATTICE_ANY},
                                  {PFM_SPLIT_SPECTRAL, PFM_SPLIT_ROUTE_LATTICE}};
  CHECK(PFM_SPLIT_ROUTE_LATTICE_ANY == 3 && PFM_SPLIT_ROUTE_LATTICE_ANY == (PFM_SPLIT_ROUTE_LATTICE | 2), "the route value");
  int n = 0, n_spectral = 0, n_voldev = 0;
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
                          for (int arm = 0; arm < N_ARMS; ++arm)
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
                              const CartPlan base = plan_cart(v, cv, p, ro, phase, N_CU); // without the argument
                              const CartPlan pl = plan_cart(v, cv, p, ro, phase, N_CU, arms[arm]);
                              const CartPlan vd = plan_cart(v, cv, p, ro, phase, N_CU, {PFM_SPLIT_VOLDEV, PFM_SPLIT_ROUTE_LATTICE});
                              ++n;
                              CHECK(!base.voldev && !base.spectral && base.supported == !split, "the default: split %d supported %d", split, (int)base.supported);
                              const bool lattice_law = split && dim == 3 && ro;
                              if (lattice_law && arm == SPECTRAL_ANY)
                                {
                                  ++n_spectral;
                                  CHECK(pl.spectral && !pl.voldev && vd.voldev && !vd.spectral && pl.supported && pl.residual == PFM_RES_3 && !pl.rows_residual &&
                                          !pl.pair && !pl.uu3() && !pl.phi4() && !pl.cells2(),
                                        "phase %d scheme %d het %d il %d sub %d fused %d level %d: spectral %d voldev %d supported %d residual %d", phase, scheme,
                                        het, il, sub, fused, level, (int)pl.spectral, (int)pl.voldev, (int)pl.supported, (int)pl.residual);
                                  CHECK(same_but_the_law(pl, vd), "phase %d scheme %d het %d il %d sub %d fused %d level %d listed %d forced %d: the spectral plan differs from the voldev plan",
                                        phase, scheme, het, il, sub, fused, level, listed, forced);
                                  CHECK(pl.grid[PFM_ZC_RES3].n_tiles > 0 && pl.tile_sel(PFM_ZC_RES3) == phase, "the residual kernel is the one cut into halves");
                                }
                              else if (lattice_law && arm == VOLDEV_ANY)
                                {
                                  ++n_voldev;
                                  CHECK(pl.voldev && !pl.spectral && same_plan(pl, vd), "phase %d scheme %d het %d il %d sub %d fused %d level %d: model 3 on route 3 is not model 3 on route 1",
                                        phase, scheme, het, il, sub, fused, level);
                                }
                              else
                                CHECK(same_plan(pl, base), "dim %d phase %d ro %d scheme %d het %d il %d sub %d fused %d level %d split %d arm %d differs from the default",
                                      dim, phase, ro, scheme, het, il, sub, fused, level, split, arm);
                            }
  printf("split route 3: %d plans, %d spectral, %d voldev\n", n, n_spectral, n_voldev);
  const int want = 3 * N_SCHEMES * 2 * 2 * 2 * 2 * 2 * 2 * 2;
  CHECK(n_spectral == want && n_voldev == want, "%d spectral and %d voldev plans, %d expected", n_spectral, n_voldev, want);
  printf(n_fail ? "split_route_any_plan: %d FAILED\n" : "split_route_any_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

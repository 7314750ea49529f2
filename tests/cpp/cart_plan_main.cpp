// The plan and the tile geometry of the cartesian launchers (cracks_amd/csrc/pfm_cart_plan.h) as a stand-alone host program
// under AddressSanitizer and UBSan: no GPU, no HIP call.  Driven by tests/test_cart_plan_host.py, once per setting of the switches
// that are read once per process; the switches that are read per call are flipped in here.
#include "pfm_cart_plan.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

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

// lattice (NX,NY,NZ) with the owned sub-box [o0, o1]
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
static CartView sub_box()
{
  const int o0[3] = {3, 2, 4}, o1[3] = {10, 7, 12};
  return box(14, 11, 16, o0, o1);
}

static void check_grid(const CartView &cv, int kernel, const char *what)
{
  const TileShape &t = tile_shape[kernel];
  const int planes = t.march < 0 ? 1 : cv.o1[t.march] - cv.o0[t.march] + 1;
  for (int forced : {0, 1, planes, planes + 5})
    for (int sel : {0, 1, 2})
      {
        CartView c = cv;
        c.tile_sel = sel;
        if (kernel < PFM_ZC_KERNELS)
          c.zc_force[kernel] = forced;
        const TileGrid g = cart_tile_grid(c, kernel, N_CU);
        const int ox = cv.o1[0] - cv.o0[0] + 1, oy = cv.o1[1] - cv.o0[1] + 1;
        CHECK(g.n_tiles == (unsigned)(g.ntx * g.nty * g.nch), "%s kernel %d: %u tiles", what, kernel, g.n_tiles);
        CHECK(g.ntx >= 1 && (g.ntx - 1) * t.tx < ox && ox <= g.ntx * t.tx, "%s kernel %d ntx %d", what, kernel, g.ntx);
        if (t.ty)
          CHECK(g.nty >= 1 && (g.nty - 1) * t.ty < oy && oy <= g.nty * t.ty, "%s kernel %d nty %d", what, kernel, g.nty);
        else
          CHECK(g.nty == 1, "%s kernel %d nty %d", what, kernel, g.nty);
        // the chunks cover the marching extent exactly: none empty, none missing
        CHECK(g.zc >= 1 && g.zc <= planes && (g.nch - 1) * g.zc < planes && planes <= g.nch * g.zc, "%s kernel %d: zc %d, %d chunks, %d planes", what,
              kernel, g.zc, g.nch, planes);
        if (t.march < 0)
          continue;
        if (kernel == PFM_ZC_UU3 && sel != 0)
          CHECK(g.zc == 1, "%s: k_cart_uu3 marches single planes in a half, zc %d", what, g.zc);
        else if (forced > 0)
          CHECK(g.zc == std::min(forced, planes), "%s kernel %d: forced %d -> %d", what, kernel, forced, g.zc);
        else
          CHECK(g.zc >= std::min(t.zc_min, planes) && g.zc <= t.zc_max, "%s kernel %d: the model picked %d", what, kernel, g.zc);
      }
}

// does a node of [lo, hi] along `axis` lie on the lattice but outside the owned box?  (node by node)
static bool touches_ghost(const CartView &cv, int axis, int lo, int hi)
{
  const int n = axis == 0 ? cv.NX : axis == 1 ? cv.NY : cv.NZ;
  for (int x = std::max(lo, 0); x <= std::min(hi, n - 1); ++x)
    if (x < cv.o0[axis] || x > cv.o1[axis])
      return true;
  return false;
}

static void check_boundary_lists(const CartView &cv, int kernel)
{
  std::vector<int32_t> list;
  CartView half2 = cv;
  half2.tile_sel = 2;
  const TileGrid g = cart_tile_grid(half2, kernel, N_CU, &list);
  const TileShape &t = tile_shape[kernel];
  CHECK(g.n_tiles == (unsigned)(g.ntx * g.nty * g.nch), "kernel %d: %u tiles", kernel, g.n_tiles);
  std::set<int32_t> in(list.begin(), list.end());
  CHECK(in.size() == list.size(), "kernel %d: a tile is listed twice", kernel);
  for (int32_t i : list)
    CHECK(i >= 0 && (unsigned)i < g.n_tiles, "kernel %d: tile %d of %u", kernel, i, g.n_tiles);
  for (int ch = 0; ch < g.nch; ++ch)
    for (int ty = 0; ty < g.nty; ++ty)
      for (int tx = 0; tx < g.ntx; ++tx)
        {
          const int i0 = cv.o0[0] + tx * t.tx, j0 = cv.o0[1] + ty * t.ty, k0 = cv.o0[2] + ch * g.zc;
          const int k1 = std::min(k0 + g.zc - 1, cv.o1[2]); // last plane of the chunk
          const bool ghost = touches_ghost(cv, 0, i0 - 1, i0 + t.tx) || touches_ghost(cv, 1, j0 - 1, j0 + t.ty) || touches_ghost(cv, 2, k0 - 1, k1 + 1);
          const int idx = tx + g.ntx * (ty + g.nty * ch);
          CHECK(ghost == (in.count(idx) == 1), "kernel %d tile (%d,%d,%d): ghost %d, listed %d", kernel, tx, ty, ch, (int)ghost, (int)in.count(idx));
        }
  // the second half over the list
  CartView c = cv;
  c.tile_sel = 2;
  (kernel == PFM_ZC_UU3 ? c.bnd_uu3 : c.bnd_res3) = list.data();
  (kernel == PFM_ZC_UU3 ? c.n_bnd_uu3 : c.n_bnd_res3) = (int)list.size();
  c.zc_res3 = g.zc;
  TileGrid h = cart_tile_grid(c, kernel, N_CU);
  CHECK(h.n_tiles == list.size() && h.zc == g.zc, "kernel %d: %u tiles over the list", kernel, h.n_tiles);
  c.zc_res3 = g.zc + 1; // a list of another chunk length is not used
  h = cart_tile_grid(c, kernel, N_CU);
  CHECK(h.n_tiles == (kernel == PFM_ZC_UU3 ? list.size() : g.n_tiles), "kernel %d: list of a stale chunk length", kernel);
  c.tile_sel = 1;
  CHECK(cart_tile_grid(c, kernel, N_CU).n_tiles == g.n_tiles, "kernel %d: the first half takes no list", kernel);
}

// ---- the routing, as the launchers had it before there was a plan: three literal tables, first match, -1 = any -------------
enum Scheme { STAGGERED, MONOLITHIC, PENALISED, KAPPA_LARGE, SPLIT, N_SCHEMES };
// the Jacobian kernels write the residual: 3-D, full assembly, and
struct RowsRule { int scheme, het, res_kernel_env, rows; };
static const RowsRule rows_table[] = {{STAGGERED, 0, 0, 1}, {-1, -1, -1, 0}};
// what runs: dim, residual_only, phase, rows_residual -> k_cart2d_cells, a residual kernel, k_cart_uu3, k_cart_phi4, the pair
struct SeqRule { int dim, ro, phase, rows, cells2, residual, uu3, phi4, pair; };
static const SeqRule seq_table[] = {{2, 0, -1, -1, 1, 0, 0, 0, 0}, {2, 1, -1, -1, 0, 1, 0, 0, 0}, {3, 1, -1, -1, 0, 1, 0, 0, 0},
                                    {3, 0, 0, 1, 0, 0, 1, 1, 1},   {3, 0, 1, 1, 0, 0, 1, 0, 0},   {3, 0, 2, 1, 0, 0, 1, 1, 0},
                                    {3, 0, 0, 0, 0, 1, 1, 1, 0},   {3, 0, 1, 0, 0, 1, 0, 0, 0},   {3, 0, 2, 0, 0, 1, 1, 1, 0}};
// which residual kernel: dim, linear scheme, whole lexicographic box by transfer, fused solution, interleaved, no wide transfers, het
struct ResRule { int dim, linear, whole, fused, il, no_wide, het, kind, flag; };
static const ResRule res_table[] = {{2, 1, -1, -1, -1, -1, -1, PFM_RES_2M, 1}, {2, 0, -1, -1, -1, -1, -1, PFM_RES_2M, 0},
                                    {3, 1, 1, 1, 0, 0, 0, PFM_RES_3X, 0},      {3, 1, 1, 1, 0, 0, 1, PFM_RES_3X, 1},
                                    {3, 1, 1, -1, -1, -1, 0, PFM_RES_3D, 0},   {3, 1, 1, -1, -1, -1, 1, PFM_RES_3D, 1},
                                    {3, 1, 0, -1, -1, -1, -1, PFM_RES_3, 1},   {3, 0, -1, -1, -1, -1, -1, PFM_RES_3, 0}};
static bool m(int rule, int value) { return rule < 0 || rule == value; }

static pfm_params params_of(int scheme)
{
  pfm_params p{};
  p.lambda = 1.0, p.mu = 1.0, p.constant_k = 1e-10, p.alpha_eps = 0.1, p.G_c = 1.0, p.alpha_biot = 0.0;
  p.timestep = 0.5, p.old_timestep = 0.5, p.old_old_timestep = 0.5, p.time = 2.0, p.timestep_number = 2;
  p.outer_solver = PFM_SOLVER_ACTIVE_SET;
  if (scheme == MONOLITHIC)
    p.outer_solver = PFM_SOLVER_SIMPLE_MONOLITHIC, p.timestep_number = 0; // (step 0: no penalty, monolithic all the same)
  if (scheme == PENALISED)
    p.gamma_penal = 10.0;
  if (scheme == KAPPA_LARGE)
    p.constant_k = 0.5;
  if (scheme == SPLIT)
    p.decompose_stress_matrix = 1;
  return p;
}

static void check_routing()
{
  // read once per process, so the driver starts the program once per setting
  const bool res_kernel_env = getenv("PFM_RES_KERNEL") != nullptr, jac_seq_env = getenv("PFM_JAC_SEQUENTIAL") != nullptr;
  const bool uu_clk_env = getenv("PFM_UU_CLK") != nullptr;
  const int phi_clk_env = !getenv("PFM_PHI_CLK") ? 0 : atoi(getenv("PFM_PHI_CLK")) == 2 ? 2 : 1;
  static const int32_t row_table[1] = {0};
  static const double lam[1] = {1.0}, sol[1] = {0.0};
  int n = 0, n_pair = 0, n_kind[5] = {0, 0, 0, 0, 0};
  for (int dim : {2, 3})
    for (int ro : {0, 1})
      for (int phase : {0, 1, 2})
        for (int scheme = 0; scheme < N_SCHEMES; ++scheme)
          for (int het : {0, 1})
            for (int il : {0, 1})
              for (int sub : {0, 1})
                for (int fused : {0, 1})
                  for (int sw = 0; sw < 16; ++sw)
                    {
                      const int level = (sw >> 3) & 1; // a level lattice of an overlay: its rows by table
                      const int no_tr = sw & 1, no_wide = (sw >> 1) & 1, one = (sw >> 2) & 1;
                      no_tr ? setenv("PFM_RES_NO_TRANSFERS", "1", 1) : unsetenv("PFM_RES_NO_TRANSFERS");
                      no_wide ? setenv("PFM_RES_NO_WIDE_TRANSFERS", "1", 1) : unsetenv("PFM_RES_NO_WIDE_TRANSFERS");
                      one ? setenv("PFM_CART2D_ONE_LAUNCH", "1", 1) : unsetenv("PFM_CART2D_ONE_LAUNCH");
                      CartView cv = dim == 2 ? whole(12, 7, 1) : sub ? sub_box() : whole(9, 5, 11);
                      if (dim == 2 && sub)
                        cv.NX += 3, cv.o0[0] += 2, cv.o1[0] += 2;
                      cv.cell_lam = cv.cell_mu = het ? lam : nullptr;
                      cv.row_of_box = level ? row_table : nullptr;
                      DevView v{};
                      v.dim = dim;
                      v.layout = il ? PFM_LAYOUT_INTERLEAVED : PFM_LAYOUT_BLOCKED;
                      v.n_nodes = cv.NX * cv.NY * cv.NZ;
                      v.n_owned = (cv.o1[0] - cv.o0[0] + 1) * (cv.o1[1] - cv.o0[1] + 1) * (cv.o1[2] - cv.o0[2] + 1);
                      v.fused_solution = fused ? sol : nullptr;
                      const pfm_params p = params_of(scheme);
                      const CartPlan pl = plan_cart(v, cv, p, ro, phase, N_CU);
                      ++n;
                      // the invariant the two copies of the predicate used to guard by comment
                      CHECK(!pl.pair || pl.rows_residual, "pair without the residual rows");
                      CHECK(!pl.rows_residual || (dim == 3 && !ro), "residual rows outside a full 3-D assembly");
                      CHECK(!pl.pair || phase == 0, "pair in a half");
                      CHECK(pl.supported == (scheme != SPLIT), "scheme %d supported %d", scheme, (int)pl.supported);
                      if (scheme == SPLIT)
                        {
                          CHECK(!pl.cells2() && !pl.uu3() && !pl.phi4() && !pl.pair && !pl.rows_residual && pl.residual == PFM_RES_NONE, "split: nothing runs");
                          continue;
                        }
                      const int linear = scheme == STAGGERED || scheme == KAPPA_LARGE;
                      int rows = 0;
                      for (const RowsRule &r : rows_table)
                        if (m(r.scheme, scheme) && m(r.het, het) && m(r.res_kernel_env, res_kernel_env))
                          {
                            rows = r.rows && dim == 3 && !ro;
                            break;
                          }
                      const SeqRule *s = nullptr;
                      for (const SeqRule &r : seq_table)
                        if (!s && m(r.dim, dim) && m(r.ro, ro) && m(r.phase, phase) && m(r.rows, rows))
                          s = &r;
                      const int whole_box = !sub && phase == 0 && !no_tr && !level;
                      const ResRule *k = nullptr;
                      for (const ResRule &r : res_table)
                        if (!k && m(r.dim, dim) && m(r.linear, linear) && m(r.whole, whole_box) && m(r.fused, fused) && m(r.il, il) &&
                            m(r.no_wide, no_wide) && m(r.het, het))
                          k = &r;
                      CHECK(s && k, "no rule");
                      if (!s || !k)
                        continue;
                      const int kind = s->residual ? k->kind : (int)PFM_RES_NONE;
                      // the pair: where the table has it, and not on a level lattice, not in turn, not with a clock
                      const bool pair = s->pair && !level && !jac_seq_env && !uu_clk_env && !phi_clk_env;
                      CHECK(pl.rows_residual == (rows != 0) && pl.pair == pair && pl.cells2() == (s->cells2 != 0) && pl.uu3() == (s->uu3 != 0) &&
                              pl.phi4() == (s->phi4 != 0) && (int)pl.residual == kind && (!s->residual || pl.residual_flag() == (k->flag != 0)),
                            "dim %d ro %d phase %d scheme %d het %d il %d sub %d fused %d sw %d: rows %d pair %d cells2 %d uu3 %d phi4 %d residual %d<%d>, "
                            "expected rows %d pair %d cells2 %d uu3 %d phi4 %d residual %d<%d>",
                            dim, ro, phase, scheme, het, il, sub, fused, sw, (int)pl.rows_residual, (int)pl.pair, (int)pl.cells2(), (int)pl.uu3(), (int)pl.phi4(),
                            (int)pl.residual, (int)pl.residual_flag(), rows, (int)pair, s->cells2, s->uu3, s->phi4, kind, k->flag);
                      CHECK(pl.interleaved == (il != 0) && pl.het == (het != 0) && pl.oldf() == !linear && pl.one_launch == (s->cells2 && one),
                            "flags: il %d het %d oldf %d one %d", (int)pl.interleaved, (int)pl.het, (int)pl.oldf(), (int)pl.one_launch);
                      // the clocked kernels exist for the blocked layout and homogeneous material, k_cart_phi4's for !OLDF
                      CHECK(pl.uu3_clock == (uu_clk_env && !il && !het) && pl.phi4_clock == ((!il && !het && linear) ? phi_clk_env : 0),
                            "il %d het %d linear %d: clocks %d %d", il, het, linear, (int)pl.uu3_clock, pl.phi4_clock);
                      // the first kernel of the sequence is the one cut into halves
                      const int first = s->cells2 ? PFM_TILES_CELLS2 : s->residual ? (dim == 2 ? PFM_ZC_RES2 : PFM_ZC_RES3) : PFM_ZC_UU3;
                      for (int kk = 0; kk < PFM_TILE_KERNELS; ++kk)
                        CHECK(pl.tile_sel(kk) == (kk == first ? phase : 0), "tile_sel of kernel %d", kk);
                      n_pair += pl.pair;
                      ++n_kind[pl.residual];
                    }
  unsetenv("PFM_RES_NO_TRANSFERS"), unsetenv("PFM_RES_NO_WIDE_TRANSFERS"), unsetenv("PFM_CART2D_ONE_LAUNCH");
  printf("routing: %d plans, %d pairs, residual kernels none/3x/3d/3/2m = %d/%d/%d/%d/%d\n", n, n_pair, n_kind[0], n_kind[1], n_kind[2], n_kind[3],
         n_kind[4]);
  CHECK((res_kernel_env || jac_seq_env || uu_clk_env || phi_clk_env) ? n_pair == 0 : n_pair > 0, "pairs: %d", n_pair);
  for (int i = 1; i < 5; ++i)
    CHECK(n_kind[i] > 0, "residual kernel %d never chosen", i);
}

int main()
{
  const CartView b1 = whole(1, 1, 1), b2 = whole(8, 4, 9), b3 = whole(9, 5, 11), b4a = whole(15, 15, 22), b4b = whole(16, 16, 23);
  const CartView b5a = whole(12, 7, 1), b5b = whole(62, 5, 1), b5c = whole(63, 5, 1), b6 = sub_box();
  const struct { const CartView *cv; const char *what; bool flat; } boxes[] = {{&b1, "(1,1,1)", false}, {&b2, "(8,4,9)", false}, {&b3, "(9,5,11)", false},
      {&b4a, "(15,15,22)", false}, {&b4b, "(16,16,23)", false}, {&b5a, "(12,7)", true}, {&b5b, "(62,5)", true}, {&b5c, "(63,5)", true}, {&b6, "sub-box", false}};
  for (const auto &b : boxes)
    for (int k = 0; k < PFM_TILE_KERNELS; ++k)
      if (b.flat == (k == PFM_ZC_RES2 || k == PFM_TILES_CELLS2))
        check_grid(*b.cv, k, b.what);
  // tile counts at the edges of a tile
  auto tiles = [](const CartView &cv, int k) { const TileGrid g = cart_tile_grid(cv, k, N_CU); return g.ntx * 100 + g.nty; };
  CHECK(tiles(b2, PFM_ZC_UU3) == 101 && tiles(b3, PFM_ZC_UU3) == 202, "k_cart_uu3: %d %d", tiles(b2, PFM_ZC_UU3), tiles(b3, PFM_ZC_UU3));
  CHECK(tiles(b3, PFM_ZC_PHI4) == 201 && tiles(b4a, PFM_ZC_PHI4) == 303, "k_cart_phi4: %d %d", tiles(b3, PFM_ZC_PHI4), tiles(b4a, PFM_ZC_PHI4));
  CHECK(tiles(b4a, PFM_ZC_RES3) == 101 && tiles(b4b, PFM_ZC_RES3) == 202, "k_cart_residual3: %d %d", tiles(b4a, PFM_ZC_RES3), tiles(b4b, PFM_ZC_RES3));
  CHECK(tiles(b5b, PFM_ZC_RES2) == 101 && tiles(b5c, PFM_ZC_RES2) == 201, "k_cart_residual2m: %d %d", tiles(b5b, PFM_ZC_RES2), tiles(b5c, PFM_ZC_RES2));
  CHECK(tiles(b5a, PFM_TILES_CELLS2) == 201 && tiles(b5c, PFM_TILES_CELLS2) == 901, "k_cart2d_cells: %d %d", tiles(b5a, PFM_TILES_CELLS2), tiles(b5c, PFM_TILES_CELLS2));
  for (int k : {(int)PFM_ZC_UU3, (int)PFM_ZC_RES3})
    for (int forced : {0, 1, 4})
      {
        CartView c = b6;
        c.zc_force[k] = forced;
        check_boundary_lists(c, k);
      }
  check_routing();
  printf(n_fail ? "cart_plan: %d FAILED\n" : "cart_plan: OK\n", n_fail);
  return n_fail ? 1 : 0;
}

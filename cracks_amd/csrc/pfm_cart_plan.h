// pfm_cart_plan.h -- what the launchers of the cartesian family do for one assembly of one lattice, decided once
// (plan_cart), and the tile geometry they share with the boundary-tile lists.  No HIP call, allocation or launch.
#pragma once
#include "pfm_internal.h"
#include "pfm_switches.h"

#include <algorithm>
#include <vector>

namespace pfm
{
  struct CartScheme
  {
    bool split;       // stress split in the matrix (cracks.cc:2294): the general family has it, the row-owner kernels do not
    bool linear;      // staggered scheme (no q-point clamps of the phase fields) without the penalty term (cracks.cc:2141-2144, 2370)
    bool kappa_large; // kappa >= 0.5
  };
  inline CartScheme cart_scheme(const pfm_params &p)
  {
    const bool mono = p.outer_solver == PFM_SOLVER_SIMPLE_MONOLITHIC;
    // the kernels' gamma_fac divides by diam^2 as well: zero or not as here, unless that division over- or underflows
    const bool penalised = ((mono && p.timestep_number < 1) ? 0.0 : p.gamma_penal) / p.timestep != 0.0;
    return {p.decompose_stress_matrix > 0 && p.timestep_number > 0, !mono && !penalised, !(p.constant_k < 0.5)};
  }

  // The 3-D law of a split assembly and where its residual -- and, bit 4 of the route, its Jacobian -- may run (pfm_set_split_model, pfm_set_split_route).  The default
  // is what a caller of neither gets: every split assembly belongs to the general family.
  struct CartSplit
  {
    int model = PFM_SPLIT_REFERENCE, route = PFM_SPLIT_ROUTE_GENERAL;
  };

  // owned nodes per tile: k_cart_uu3 T3X x T3Y, k_cart_phi4 PN x PN, k_cart_residual3* RNX x RNY, k_cart_residual2m R2N, k_cart2d_cells O2 x O2
  constexpr int T3X = 8, T3Y = 4, PN = 7, RNX = 15, RNY = 15, R2N = 62, O2 = 7;
  constexpr int PFM_TILES_CELLS2 = PFM_ZC_KERNELS, PFM_TILE_KERNELS = PFM_ZC_KERNELS + 1; // the PFM_ZC_* kernels, then k_cart2d_cells
  struct TileShape
  {
    int tx, ty, march;          // tile (ty = 0: none along y), axis of the chunks (-1: none)
    int zc_min, zc_max, per_cu; // range of the chunk model, resident workgroups per CU (k_cart_residual2m: one wave each)
  };
  constexpr TileShape tile_shape[PFM_TILE_KERNELS] = {{T3X, T3Y, 2, 8, 48, 2}, {PN, PN, 2, 6, 48, 2}, {RNX, RNY, 2, 4, 24, 2},
                                                      {R2N, 0, 1, 4, 64, 8},   {O2, O2, -1, 0, 0, 0}};
  constexpr int PFM_PAIR_LDS_BYTES = 64 * 1280; // LDS of a k_cart_phi4 workgroup (64 granules; 79,472 B are 63)

  // z-chunk length of a marching kernel over `tiles` columns of `planes` node planes, one redundant cell layer per chunk.
  // Time model: workgroups are dispatched as slots free up, so the launch takes about (wgs / slots + 1/2) workgroup durations,
  // and a workgroup's duration is proportional to its zc + 1 cell layers.  The longest chunk within 1 % of the optimum.
  inline int choose_zchunk(long long tiles, int planes, int zc_min, int zc_max, int per_cu, int n_cu)
  {
    const double slots = (double)per_cu * n_cu;
    const int lo = std::max(1, std::min(zc_min, planes)), hi = std::min(zc_max, planes);
    auto t = [&](int zc) { return ((double)tiles * ((planes + zc - 1) / zc) / slots + 0.5) * (zc + 1); };
    double tmin = 1e300;
    for (int zc = lo; zc <= hi; ++zc)
      tmin = std::min(tmin, t(zc));
    int best = lo;
    for (int zc = lo; zc <= hi; ++zc)
      if (t(zc) <= 1.01 * tmin)
        best = zc;
    return best;
  }

  struct TileGrid
  {
    int ntx, nty, zc, nch; // tiles in the plane; nodes per chunk along the marching axis, chunks (1, 1 without a march)
    unsigned n_tiles;      // ntx nty nch, or the length of the list of boundary tiles
  };
  // The tiles of `kernel` (PFM_ZC_*, PFM_TILES_CELLS2) over the owned box of cv, for cv.tile_sel.  Chunk length: cv.zc_force,
  // else the tuning variable, else the model; forced lengths are clamped to [1, planes].  k_cart_uu3 marches single planes in
  // the halves of an overlapped assembly; the second half runs over CartView::bnd_* where the context has that list
  // (k_cart_residual3: for today's chunk length).  boundary: gets the tiles that read a ghost node appended.
  inline TileGrid cart_tile_grid(const CartView &cv, int kernel, int n_cu, std::vector<int32_t> *boundary = nullptr)
  {
    const TileShape &t = tile_shape[kernel];
    const int ox = cv.o1[0] - cv.o0[0] + 1, oy = cv.o1[1] - cv.o0[1] + 1, planes = t.march < 0 ? 1 : cv.o1[t.march] - cv.o0[t.march] + 1;
    TileGrid g{(ox + t.tx - 1) / t.tx, t.ty ? (oy + t.ty - 1) / t.ty : 1, 1, 1, 0};
    const int forced = t.march < 0 ? 1 : cv.zc_force[kernel] > 0 ? cv.zc_force[kernel] : switches().zc[kernel];
    if (t.march >= 0 && !(kernel == PFM_ZC_UU3 && cv.tile_sel != 0))
      g.zc = forced > 0 ? std::max(1, std::min(forced, planes)) : choose_zchunk((long long)g.ntx * g.nty, planes, t.zc_min, t.zc_max, t.per_cu, n_cu);
    g.nch = (planes + g.zc - 1) / g.zc;
    g.n_tiles = (unsigned)(g.ntx * g.nty * g.nch);
    for (int i = 0; boundary && i < (int)g.n_tiles; ++i)
      {
        const int i0 = cv.o0[0] + i % g.ntx * t.tx, j0 = cv.o0[1] + i / g.ntx % g.nty * t.ty, kA = cv.o0[2] + i / (g.ntx * g.nty) * g.zc;
        if (cart_range_has_ghost(cv, 0, i0 - 1, i0 + t.tx) || cart_range_has_ghost(cv, 1, j0 - 1, j0 + t.ty) ||
            cart_range_has_ghost(cv, 2, kA - 1, std::min(kA + g.zc, cv.o1[2] + 1)))
          boundary->push_back(i);
      }
    if (cv.tile_sel == 2 && kernel == PFM_ZC_UU3 && cv.bnd_uu3)
      g.n_tiles = (unsigned)cv.n_bnd_uu3;
    if (cv.tile_sel == 2 && kernel == PFM_ZC_RES3 && cv.bnd_res3 && cv.zc_res3 == g.zc)
      g.n_tiles = (unsigned)cv.n_bnd_res3;
    return g;
  }

  enum CartResidual { PFM_RES_NONE, PFM_RES_3X, PFM_RES_3D, PFM_RES_3, PFM_RES_2M }; // k_cart_residual3x<het>, 3d<het>, 3<linear> (CartPlan::voldev, voldev_jac: 3<false, true>; spectral: 3<false, false, true>), 2m<linear>
  struct CartPlan
  {
    int dim = 0, phase = 0; // 0: the whole assembly; 1, 2: the halves of pfm_assemble_overlapped (ghost import in between)
    bool residual_only = false, supported = false; // not supported (stress split): the general family takes the assembly
    // ... but for the residual-only assembly of a 3-D context under PFM_SPLIT_VOLDEV on PFM_SPLIT_ROUTE_LATTICE: the law is a few
    // scalar statements on the strain and runs in k_cart_residual3<false, true>, for every scheme, cut into halves as an
    // unsplit PFM_RES_3 is (k_cart_uu3 and k_cart_phi4 have no split form: a full assembly is voldev_jac's, below, or unsupported)
    bool voldev = false;
    // ... and under PFM_SPLIT_SPECTRAL on PFM_SPLIT_ROUTE_LATTICE_ANY: the eigen split of pfm_split3.h at the q-points of
    // k_cart_residual3<false, false, true>.  In every other field the plan is the voldev plan of the same lattice and phase.
    bool spectral = false;
    // ... and the FULL assembly of a 3-D box under PFM_SPLIT_VOLDEV on a route with PFM_SPLIT_ROUTE_LATTICE_JACOBIAN's bit 4:
    // k_cart_split3_jac (pfm_cart_split3.hip) writes the matrix values with the law at its q-points, over the tiles and chunks
    // of k_cart_uu3 (grid[PFM_ZC_UU3]), and k_cart_residual3<false, true> writes residual_pde, cut into halves as an unsplit
    // PFM_RES_3 is.  The identity R_u = pressure part - K_uu u does not hold when d_mat != d_rhs: rows_residual and pair are
    // false for every scheme.  On a level lattice of the 3-D overlay (CartView::row_of_box) only with bit 8 of the route
    // (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS, _ALL_LEVELS): k_cart_split3_jac<NCOL, true> over grid[PFM_ZC_UU3] of that level.
    bool voldev_jac = false;
    // ... with bit 16 of the route (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE, _ALL_SPARSE) on a box: the
    // law only where it differs from the unsplit one.  k_cart_split3_mark finds the cells with a compressed q-point, the
    // unsplit k_cart_uu3 and k_cart_phi4 write every row, the sparse form of k_cart_split3_jac writes the rows at those cells
    // again (launch_assemble_cart).  In every other field the plan is the voldev_jac plan of the route without the bit.
    // On a level lattice only with bits 8, 16 and 32 (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE, _ALL_LEVELS_SPARSE): the same
    // sequence with the level forms of the mark kernel and of the sparse kernel, per level.
    bool voldev_sparse = false;
    bool linear = false, interleaved = false, het = false; // scheme; layout; per-cell Lame coefficients (CartView::cell_lam)
    // Full 3-D assembly, linear scheme: every residual row is an exact function of its own matrix row (R_u = pressure part -
    // K_uu u, R_phi = G_c/eps mass - K_phiphi phi), so the Jacobian kernels write it and no residual kernel runs (2.1 of 15.8 ms
    // at 216^3).  PFM_RES_KERNEL=1 keeps the quadrature kernel; the heterogeneous (u,u) variant has no registers left for it.
    bool rows_residual = false;
    // ... side by side on two streams: the caller forks, joins and applies the deferred patches (CartView::patch_*), the (u,u)
    // kernel takes the LDS allocation of the other.  Not in a half, not on a level lattice, not in another mode.
    bool pair = false;
    // ... of a pair into a kept (u,u) block (pfm_values_keep_uu_block; plan_keep_uu): k_cart_uu3 in its form without the
    // residual rows, which returns at once when the block is current (CartView::uu_stale), and behind it on the same stream
    // the quadrature kernel `u_rows` (PFM_RES_3D or PFM_RES_3, what `residual` would be without rows_residual) storing the
    // displacement rows of residual_pde alone: those rows have the same bits whether the block was written or kept.
    // k_cart_phi4 writes the phase-field rows as in every pair.
    bool keep_uu = false;
    CartResidual u_rows = PFM_RES_NONE;
    CartResidual residual = PFM_RES_NONE; // the residual kernel that runs
    bool one_launch = false;              // k_cart2d_cells<2> instead of <0> + <1>
    // phase clocks (profiling) exist for the blocked layout, homogeneous material and k_cart_phi4<!OLDF>: nothing else is clocked
    bool uu3_clock = false;
    int phi4_clock = 0;                   // 1: cycles per phase, 2: per role
    TileGrid grid[PFM_TILE_KERNELS] = {}; // of the kernels that run
    // What runs, in this order: k_cart2d_cells alone, or the residual kernel, k_cart_uu3, k_cart_phi4.  The first is the one
    // cut into interior / boundary tiles; the Jacobian kernels behind a residual kernel, and k_cart_phi4 always (it patches
    // (u,u) diagonals), run whole in the second half.
    bool cells2() const { return supported && dim == 2 && !residual_only; }
    bool uu3() const { return supported && dim == 3 && !residual_only && !voldev_jac && (rows_residual || phase != 1); }
    bool split3_jac() const { return supported && voldev_jac && phase != 1; } // k_cart_split3_jac: whole, behind the residual kernel
    bool phi4() const { return uu3() && phase != 1; }
    bool oldf() const { return !linear; } // k_cart_phi4<OLDF>: q-point loops, old phase fields in the nodal ring
    bool residual_flag() const { return residual <= PFM_RES_3D ? het : linear; }
    int tile_sel(int kernel) const
    {
      return kernel == (cells2() ? PFM_TILES_CELLS2 : residual == PFM_RES_2M ? PFM_ZC_RES2 : residual ? PFM_ZC_RES3 : PFM_ZC_UU3) ? phase : 0;
    }
  };

  // No side effects: what lattice cv of view v, the parameters and the switches say about this assembly.
  inline CartPlan plan_cart(const DevView &v, const CartView &cv, const pfm_params &p, int residual_only, int phase, int n_cu,
                            const CartSplit &split = CartSplit())
  {
    const Switches &sw = switches();
    const CartScheme sc = cart_scheme(p);
    CartPlan pl;
    pl.dim = v.dim, pl.phase = phase, pl.residual_only = residual_only != 0;
    const bool lattice_law = sc.split && v.dim == 3 && pl.residual_only; // a split residual that the row-owner kernel can carry
    const int res_route = split.route & PFM_SPLIT_ROUTE_LATTICE_ANY; // bits 4 and 8 (the Jacobian) say nothing about the residual-only call
    pl.voldev = lattice_law && split.model == PFM_SPLIT_VOLDEV &&
                (res_route == PFM_SPLIT_ROUTE_LATTICE || res_route == PFM_SPLIT_ROUTE_LATTICE_ANY);
    pl.spectral = lattice_law && split.model == PFM_SPLIT_SPECTRAL && res_route == PFM_SPLIT_ROUTE_LATTICE_ANY;
    pl.voldev_jac = sc.split && v.dim == 3 && !pl.residual_only && split.model == PFM_SPLIT_VOLDEV && (split.route & 4) != 0 &&
                    (split.route & PFM_SPLIT_ROUTE_LATTICE) != 0 && (!cv.row_of_box || (split.route & 8) != 0);
    pl.voldev_sparse = pl.voldev_jac && (split.route & 16) != 0 && (!cv.row_of_box || (split.route & 32) != 0);
    pl.supported = (!sc.split || pl.voldev || pl.spectral || pl.voldev_jac) && (v.dim == 2 || v.dim == 3);
    if (!pl.supported)
      return pl;
    pl.linear = sc.linear, pl.interleaved = v.layout == PFM_LAYOUT_INTERLEAVED, pl.het = cv.cell_lam != nullptr;
    pl.rows_residual = v.dim == 3 && !pl.residual_only && sc.linear && !sc.kappa_large && !sw.res_kernel && !pl.het && !pl.voldev_jac;
    pl.pair = pl.rows_residual && phase == 0 && !cv.row_of_box && !sw.jac_sequential && !sw.uu_clock && !sw.phi_clock;
    pl.one_launch = pl.cells2() && Switches::cart2d_one_launch();
    // the whole lexicographic box of a single rank, every byte offset of a node below 4 GiB: planes by transfer
    const bool whole_lex = cv.owned_lex && cv.o0[0] == 0 && cv.o0[1] == 0 && cv.o0[2] == 0 && cv.o1[0] == cv.NX - 1 &&
                           cv.o1[1] == cv.NY - 1 && cv.o1[2] == cv.NZ - 1 && phase == 0 && !cv.row_of_box &&
                           (long long)v.n_nodes == (long long)cv.NX * cv.NY * cv.NZ && v.n_owned == v.n_nodes &&
                           (long long)v.n_nodes * 32 < (1LL << 32) && !Switches::res_no_transfers();
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
          pl.grid[k] = cart_tile_grid(sel, k, n_cu);
        }
    return pl;
  }

  // CartPlan::keep_uu on the plan of a pair (plan_assembly decides whether the promise applies)
  inline void plan_keep_uu(CartPlan &pl, const DevView &v, const CartView &cv, int n_cu)
  {
    if (!pl.pair)
      return;
    const bool whole_lex = cv.owned_lex && cv.o0[0] == 0 && cv.o0[1] == 0 && cv.o0[2] == 0 && cv.o1[0] == cv.NX - 1 &&
                           cv.o1[1] == cv.NY - 1 && cv.o1[2] == cv.NZ - 1 && (long long)v.n_nodes == (long long)cv.NX * cv.NY * cv.NZ &&
                           v.n_owned == v.n_nodes && (long long)v.n_nodes * 32 < (1LL << 32) && !Switches::res_no_transfers();
    pl.keep_uu = true;
    pl.u_rows = whole_lex ? PFM_RES_3D : PFM_RES_3; // (PFM_RES_3X reads the caller's vector in place: not in a full assembly)
    CartView sel = cv;
    sel.tile_sel = 0;
    pl.grid[PFM_ZC_RES3] = cart_tile_grid(sel, PFM_ZC_RES3, n_cu);
  }
} // namespace pfm

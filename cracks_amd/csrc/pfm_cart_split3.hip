// pfm_cart_split3.hip — gfx950 Jacobian kernel of the cartesian family for the volumetric-deviatoric stress split
// (PFM_SPLIT_VOLDEV on PFM_SPLIT_ROUTE_LATTICE_JACOBIAN / _ALL; CartPlan::voldev_jac).
//
//   ROW OWNER, as pfm_cart.hip: work is assigned by owned node.  A lane owns one node and forms its four matrix rows one
//   after the other -- (node, u_x), (node, u_y), (node, u_z), (node, phi) -- each completely in registers (27 neighbour slots
//   x 3 or 4 column components), and writes every CSR value once: no atomics, no zeroing pass, bitwise reproducible, and a
//   row does not depend on how the mesh is cut over ranks or into the halves of an overlapped assembly.
//
//   PLAIN Q-POINT FORM.  The tangent of the law is isotropic at every q-point, g C+ + d_mat C- = a I(x)I + 2 b I_s with
//   b = mu g and a = voldev_tangent_a (pfm_split3.h), but a carries h(tr E), which is no polynomial: the rows are summed
//   q-point by q-point over the (up to) eight cells of the node, the statements of the VOLDEV branches of
//   k_assemble_general (pfm_kernels.hip) with the shape gradients of a cartesian cell put in.  Nothing is staged in LDS and
//   there is no barrier; the nodal values of a cell are read once per row and cell (they stay in L1/L2 between the rows).
//
//   TRACE SIGN.  h and tr- come from tr E = gu[0][0] + gu[1][1] + gu[2][2] with the gradients formed by the statements of
//   k_cart_residual3<false, true> (line_setup / the x-stage below), through split3::voldev: the displacement rows, the
//   phase-field row and the residual kernel take the sign from the same statement on the same operands.  Where tr E is zero
//   up to rounding the matrix is not determined (include/pfm_assemble.h).
//
//   LEVEL FORM (template parameter LEVEL; PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS / _ALL_LEVELS): the same rows on one
//   refinement level's lattice of a 3-D overlay.  The rows of the launch are the regular rows of that level
//   (CartView::row_of_box; -1: the lane passes the node by), slots come from the overlay's nbr_mask / row_perm, Lame
//   coefficients and cell sizes are the level's.  The box instantiations are the parent's instruction for instruction.
//
//   SPARSE FORM (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE / _ALL_SPARSE; CartPlan::voldev_sparse): the law is the unsplit law wherever
//   tr E >= 0, and a row depends on the (up to) eight cells of its node alone.  k_cart_split3_mark writes one byte per lattice
//   cell (1: a q-point of the cell is compressed, by sj_line_setup / sj_trace / split3::voldev, the statements of the rows),
//   flags the tile-chunks that own a vertex of such a cell and counts the cells; the unsplit k_cart_uu3 and k_cart_phi4 write
//   every row (launch_assemble_cart, pfm_cart.hip); k_cart_split3_jac<NCOL, false, true> then writes the rows of the nodes at
//   compressed cells again, by the same sj_row calls: those rows are the bytes of the plain form, every other row is the
//   unsplit kernels'.  No compaction pass, no host read-back, no floating-point atomics.
//
//   SPARSE LEVEL FORM (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE / _ALL_LEVELS_SPARSE; voldev_sparse on a lattice with
//   CartView::row_of_box): both of the above on one level lattice of a 3-D overlay.  k_cart_split3_mark<true> takes the cells
//   whose eight vertices all exist on the level, flags the tile-chunks that own a regular row among them and counts by the rule
//   of the level form; the unsplit level kernels write every regular row; k_cart_split3_jac<NCOL, true, true> writes the regular
//   rows at compressed cells again: the bytes of the level form.
//
// Tiles: those of k_cart_uu3 (T3X x T3Y owned nodes, z-chunks of CartPlan::grid[PFM_ZC_UU3]); a workgroup is one wave, its 64
// lanes two node planes of the tile, marching up its chunk two planes at a time.
#include "pfm_internal.h"
#include "pfm_cart_plan.h"
#include "pfm_split3.h"

#include <hip/hip_runtime.h>
#include <type_traits>

namespace pfm
{
  namespace
  {
    struct SjScal // per-launch scalars derived from pfm_params
    {
      double lam, mu, kappa, eps, Gc, p, aB1, gamma_fac, tfac, d_mat;
      double ih[3], vol;
      int monolithic, use_old;
    };

    SjScal make_sj_scal(const pfm_params &prm, const CartView &cv)
    {
      SjScal s{};
      s.lam = prm.lambda;
      s.mu = prm.mu;
      s.kappa = prm.constant_k;
      s.eps = prm.alpha_eps;
      s.Gc = prm.G_c;
      s.p = prm.pressure;
      s.aB1 = prm.alpha_biot - 1.0;
      double gamma = prm.gamma_penal;
      if (prm.outer_solver == PFM_SOLVER_SIMPLE_MONOLITHIC && prm.timestep_number < 1)
        gamma = 0.0; // cracks.cc:2141-2144
      double diam2 = 0.0;
      s.vol = 1.0;
      for (int d = 0; d < 3; ++d)
        {
          diam2 += cv.h[d] * cv.h[d];
          s.ih[d] = 1.0 / cv.h[d];
          s.vol *= cv.h[d];
        }
      s.gamma_fac = gamma / prm.timestep * 1.0 / diam2; // cracks.cc:2370, 2419
      s.tfac = (prm.time - (prm.time - prm.old_timestep - prm.old_old_timestep)) /
               (prm.time - prm.old_timestep - (prm.time - prm.old_timestep - prm.old_old_timestep));
      s.d_mat = prm.decompose_stress_matrix;
      s.monolithic = prm.outer_solver == PFM_SOLVER_SIMPLE_MONOLITHIC;
      s.use_old = prm.use_old_timestep_pf;
      return s;
    }

    template <int N, class F>
    __device__ __forceinline__ __attribute__((always_inline)) void sj_for(F &&f)
    {
      if constexpr (N > 0)
        {
          sj_for<N - 1>(f);
          f(std::integral_constant<int, N - 1>{});
        }
    }

    // 1-D Gauss(3) point and weight on [0,1] for a run-time (wave-uniform) index: the values of make_tab1d (pfm_cart.hip)
    __device__ __forceinline__ double sj_gx(int q) { return q == 0 ? 0.5 - 0.5 * 0.7745966692414834 : (q == 1 ? 0.5 : 0.5 + 0.5 * 0.7745966692414834); }
    __device__ __forceinline__ double sj_gw(int q) { return q == 1 ? 8.0 / 18.0 : 5.0 / 18.0; }

    __device__ __forceinline__ int sj_local_id(const CartView &cv, int i, int j, int k)
    {
      if (cv.owned_lex && i >= cv.o0[0] && i <= cv.o1[0] && j >= cv.o0[1] && j <= cv.o1[1] && k >= cv.o0[2] && k <= cv.o1[2])
        return (i - cv.o0[0]) + (cv.o1[0] - cv.o0[0] + 1) * ((j - cv.o0[1]) + (cv.o1[1] - cv.o0[1] + 1) * (k - cv.o0[2]));
      return cv.local_of_box[i + (long long)cv.NX * (j + (long long)cv.NY * k)];
    }

    // nodal values of the eight vertices of cell (ci, cj, ck): U[f][vx + 2 vy + 4 vz], f = u_x u_y u_z phi phi_old phi_oldold
    __device__ __forceinline__ void sj_load_cell(const DevView &v, const CartView &cv, int ci, int cj, int ck, double (&U)[6][8])
    {
#pragma unroll
      for (int b = 0; b < 8; ++b)
        {
          const int n = sj_local_id(cv, ci + (b & 1), cj + ((b >> 1) & 1), ck + (b >> 2));
          const bool in = n >= 0;
          U[0][b] = in ? v.u[0][n] : 0.0;
          U[1][b] = in ? v.u[1][n] : 0.0;
          U[2][b] = in ? v.u[2][n] : 0.0;
          U[3][b] = in ? v.phi[n] : 0.0;
          U[4][b] = in ? v.phi_old[n] : 0.0;
          U[5][b] = in ? v.phi_oldold[n] : 0.0;
        }
    }

    // Along x every interpolated quantity of a trilinear field is linear: its value at x-vertex 0 and its x-difference on
    // the line (q_y, q_z).  The statements of k_cart_residual3 (pfm_cart.hip), field by field.
    struct SjLine
    {
      double L0[6], dL[6], Dz0[4], dDz[4], Dx[4], Dy0[4], dDy[4];
    };
    __device__ __forceinline__ void sj_line_setup(const double (&U)[6][8], double eta, double zeta, const double (&ih)[3], SjLine &ln)
    {
#pragma unroll
      for (int f = 0; f < 6; ++f)
        {
          const double a00 = U[f][0], a10 = U[f][1], a01 = U[f][2], a11 = U[f][3];
          const double b00 = U[f][4], b10 = U[f][5], b01 = U[f][6], b11 = U[f][7];
          const double lo0 = fma(eta, a01 - a00, a00), lo1 = fma(eta, a11 - a10, a10);
          const double hi0 = fma(eta, b01 - b00, b00), hi1 = fma(eta, b11 - b10, b10);
          const double d0 = hi0 - lo0, d1 = hi1 - lo1;
          ln.L0[f] = fma(zeta, d0, lo0);
          ln.dL[f] = fma(zeta, d1, lo1) - ln.L0[f];
          if (f < 4)
            {
              ln.Dz0[f] = ih[2] * d0;
              ln.dDz[f] = ih[2] * (d1 - d0);
              ln.Dx[f] = ih[0] * ln.dL[f];
              const double s0 = a01 - a00, t0 = b01 - b00, s1 = a11 - a10, t1 = b11 - b10;
              const double g0 = fma(zeta, t0 - s0, s0), g1 = fma(zeta, t1 - s1, s1);
              ln.Dy0[f] = ih[1] * g0;
              ln.dDy[f] = ih[1] * (g1 - g0);
            }
        }
    }

    // g(q) = (1 - kappa) pf_extra^2 + kappa from the old phase fields (cracks.cc:2262-2277)
    __device__ __forceinline__ double sj_degradation(const SjLine &ln, double xi, const SjScal &S, double &pfo_out)
    {
      double pfo = fma(xi, ln.dL[4], ln.L0[4]);
      double pfoo = fma(xi, ln.dL[5], ln.L0[5]);
      if (S.monolithic)
        {
          pfo = fmax(0.0, pfo);
          pfoo = fmax(0.0, pfoo);
        }
      double pfx = pfoo + S.tfac * (pfo - pfoo);
      if (pfx <= 0.0)
        pfx = 0.0;
      if (pfx >= 1.0)
        pfx = 1.0;
      if (S.use_old)
        pfx = pfo;
      pfo_out = pfo;
      return (1 - S.kappa) * pfx * pfx + S.kappa;
    }

    // tr E at the q-point: the one statement every kernel of the law takes its sign from
    __device__ __forceinline__ double sj_trace(const SjLine &ln, double xi, double &g00, double &g11, double &g22)
    {
      g00 = ln.Dx[0];
      g11 = fma(xi, ln.dDy[1], ln.Dy0[1]);
      g22 = fma(xi, ln.dDz[2], ln.Dz0[2]);
      return g00 + g11 + g22;
    }

    // what the rows need of one q-point (k_assemble_general, VOLDEV: the slots O_GW .. O_AW), JxW folded in
    struct SjPoint
    {
      double gw, aw;            // g JxW; a JxW of the tangent a I(x)I + 2 (mu g) I_s
      double cpu, cdiv, cpp;    // 2 (1 - kappa) pf JxW; 2 (alpha_B - 1) p pf JxW; (phi,phi) mass weight with the penalty term
      double cgg;               // G_c eps JxW
      double s00, s11, s22, s01, s02, s12; // sigma+
      bool compressed;          // h(tr E) == 0
    };
    template <bool FULL>
    __device__ __forceinline__ void sj_point(const SjLine &ln, double xi, double JxW, double lam, double mu, const SjScal &S, SjPoint &P)
    {
      double pfo, g00, g11, g22;
      const double g = sj_degradation(ln, xi, S, pfo);
      const double trE = sj_trace(ln, xi, g00, g11, g22);
      const split3::VolDev V = split3::voldev(trE, lam, mu);
      P.compressed = V.h == 0.0;
      P.gw = g * JxW;
      P.aw = split3::voldev_tangent_a(V, lam, mu, g, S.d_mat) * JxW;
      if constexpr (FULL)
        {
          double pf = fma(xi, ln.dL[3], ln.L0[3]);
          if (S.monolithic)
            pf = fmax(0.0, pf);
          const bool pen_on = !((pf - pfo) < 0.0); // cracks.cc:2311-2315
          const double g01 = fma(xi, ln.dDy[0], ln.Dy0[0]), g02 = fma(xi, ln.dDz[0], ln.Dz0[0]);
          const double g10 = ln.Dx[1], g12 = fma(xi, ln.dDz[1], ln.Dz0[1]);
          const double g20 = ln.Dx[2], g21 = fma(xi, ln.dDy[2], ln.Dy0[2]);
          const double t01 = g01 + g10, t02 = g02 + g20, t12 = g12 + g21;
          P.s00 = split3::voldev_sigma_plus(V, mu, g00, true);
          P.s11 = split3::voldev_sigma_plus(V, mu, g11, true);
          P.s22 = split3::voldev_sigma_plus(V, mu, g22, true);
          P.s01 = mu * t01, P.s02 = mu * t02, P.s12 = mu * t12;
          const double spE = fma(P.s00, g00, fma(P.s11, g11, P.s22 * g22)) + fma(P.s01, t01, fma(P.s02, t02, P.s12 * t12));
          P.cpu = 2.0 * (1 - S.kappa) * pf * JxW;
          P.cdiv = 2.0 * S.aB1 * S.p * pf * JxW;
          P.cpp = (((1 - S.kappa) * spE + S.Gc / S.eps) - 2.0 * S.aB1 * S.p * trE) * JxW + (pen_on ? S.gamma_fac * JxW : 0.0);
          P.cgg = S.Gc * S.eps * JxW;
        }
    }

    // shape data of a cartesian cell at a q-point: gradient of vertex (bx, by, bz) = (sx GX[by][bz], sy GY[bx][bz], sz GZ[bx][by]),
    // s = +1 for the upper vertex along the axis and -1 for the lower; value X[bx] YZ[by][bz]
    struct SjShape
    {
      double X[2], YZ[2][2], GX[2][2], GY[2][2], GZ[2][2];
    };
    __device__ __forceinline__ void sj_shape(double xi, double eta, double zeta, const double (&ih)[3], SjShape &H)
    {
      const double Y[2] = {1.0 - eta, eta}, Z[2] = {1.0 - zeta, zeta};
      H.X[0] = 1.0 - xi, H.X[1] = xi;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          {
            H.YZ[i][k] = Y[i] * Z[k];
            H.GX[i][k] = ih[0] * H.YZ[i][k];
            H.GY[i][k] = ih[1] * (H.X[i] * Z[k]);
            H.GZ[i][k] = ih[2] * (H.X[i] * Y[k]);
          }
    }
    template <int B>
    __device__ __forceinline__ void sj_grad(const SjShape &H, double (&g)[3])
    {
      constexpr int bx = B & 1, by = (B >> 1) & 1, bz = B >> 2;
      g[0] = bx ? H.GX[by][bz] : -H.GX[by][bz];
      g[1] = by ? H.GY[bx][bz] : -H.GY[bx][bz];
      g[2] = bz ? H.GZ[bx][by] : -H.GZ[bx][by];
    }
    template <int B>
    __device__ __forceinline__ double sj_value(const SjShape &H)
    {
      return H.X[B & 1] * H.YZ[(B >> 1) & 1][B >> 2];
    }

    // mean |diagonal| of the element matrix of one cell: deal.II's placeholder for a constrained row whose own diagonal
    // entry of that cell vanishes (k_assemble_general: dsum / 32).  Rare (kappa = 0 next to a fully broken cell).
    __device__ __forceinline__ double sj_cell_diag_mean(const double (&U)[6][8], double lam, double mu, const SjScal &S)
    {
      double D[8][4];
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          D[b][c] = 0.0;
#pragma unroll 1
      for (int p = 0; p < 9; ++p)
        {
          const int qy = p % 3, qz = p / 3;
          const double eta = sj_gx(qy), zeta = sj_gx(qz);
          SjLine ln;
          sj_line_setup(U, eta, zeta, S.ih, ln);
#pragma unroll 1
          for (int qx = 0; qx < 3; ++qx)
            {
              const double xi = sj_gx(qx), JxW = S.vol * (sj_gw(qx) * sj_gw(qy) * sj_gw(qz));
              SjPoint P;
              sj_point<true>(ln, xi, JxW, lam, mu, S, P);
              SjShape H;
              sj_shape(xi, eta, zeta, S.ih, H);
              const double mgw = mu * P.gw;
              sj_for<8>([&](auto Bc) __attribute__((always_inline)) {
                constexpr int b = decltype(Bc)::value;
                double gb[3];
                sj_grad<b>(H, gb);
                const double Nb = sj_value<b>(H), t = gb[0] * gb[0] + gb[1] * gb[1] + gb[2] * gb[2];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                  D[b][c] += (P.aw * gb[c]) * gb[c] + (mgw * gb[c]) * gb[c] + mgw * t;
                D[b][3] += (P.cpp * Nb) * Nb + P.cgg * t;
              });
            }
        }
      double dsum = 0.0;
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          dsum += fabs(D[b][c]);
      return dsum / 32.0;
    }

    struct SjArgs
    {
      DevView v;
      CartView cv;
      SjScal S;
      double *vals_uu, *vals_up, *vals_pu, *vals_pp; // blocked layout; interleaved: vals_uu is the one block
      int *n_compressed;                             // cells with a compressed q-point, counted by the owner of their vertex 0
      int zc;
    };
    // what the SPARSE form (CartPlan::voldev_sparse) takes on top, written by k_cart_split3_mark in front of its launch -- an
    // argument of its own: the kernel arguments of the plain instantiations are the parent's byte for byte
    struct SjSparseArgs
    {
      const uint8_t *cell_comp; // [(NX-1)(NY-1)(NZ-1)] lattice cell order: 1 = the cell has a compressed q-point
      const int *tile_flag;     // [ntx nty nch] of grid[PFM_ZC_UU3]: 1 = the tile-chunk owns a vertex of such a cell
      int *n_rows;              // nodes whose four rows this launch recomputed
    };

    // One row of the node at (gi, gj, gk): COMP < 3 the displacement row (node, COMP) with its three (u,u) columns per slot,
    // COMP == 3 the phase-field row with (phi,u) and (phi,phi).  NCOL: 3 blocked, 4 interleaved.
    template <int COMP, int NCOL>
    __device__ __forceinline__ void sj_row(const SjArgs &A, int gi, int gj, int gk, int row, unsigned row_flag)
    {
      const DevView &v = A.v;
      const CartView &cv = A.cv;
      const SjScal &S = A.S;
      constexpr bool PHI = COMP == 3;
      constexpr int NC = PHI ? 4 : 3;
      double acc[27][NC];
#pragma unroll
      for (int o = 0; o < 27; ++o)
#pragma unroll
        for (int d = 0; d < NC; ++d)
          acc[o][d] = 0.0;
      const bool rcon = (row_flag >> COMP) & 1u;
      double ph = 0.0;       // placeholder diagonal of a constrained row: sum over the cells of |K_e,aa| ...
      unsigned need_avg = 0; // ... or, where that vanishes, of the mean |diagonal| of the element matrix
      bool any_compressed = false;

      sj_for<8>([&](auto Ec) __attribute__((always_inline)) {
        // cell e of the node: the node is its vertex (1 - ex, 1 - ey, 1 - ez)
        constexpr int e = decltype(Ec)::value, ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
        constexpr int a = (1 - ex) + 2 * (1 - ey) + 4 * (1 - ez);
        const int ci = gi - 1 + ex, cj = gj - 1 + ey, ck = gk - 1 + ez;
        if (ci >= 0 && ci < cv.NX - 1 && cj >= 0 && cj < cv.NY - 1 && ck >= 0 && ck < cv.NZ - 1)
          {
            double lam = S.lam, mu = S.mu;
            if (cv.cell_lam) // heterogeneous material, cracks.cc:2207-2216
              {
                const long long cidx = ci + (long long)(cv.NX - 1) * (cj + (long long)(cv.NY - 1) * ck);
                lam = cv.cell_lam[cidx];
                mu = cv.cell_mu[cidx];
              }
            double U[6][8];
            sj_load_cell(v, cv, ci, cj, ck, U);
            double dcell = 0.0; // this cell's part of the row's diagonal entry
#pragma unroll 1
            for (int p = 0; p < 9; ++p)
              {
                const int qy = p % 3, qz = p / 3;
                const double eta = sj_gx(qy), zeta = sj_gx(qz);
                SjLine ln;
                sj_line_setup(U, eta, zeta, S.ih, ln);
#pragma unroll 1
                for (int qx = 0; qx < 3; ++qx)
                  {
                    const double xi = sj_gx(qx), JxW = S.vol * (sj_gw(qx) * sj_gw(qy) * sj_gw(qz));
                    SjPoint P;
                    sj_point<PHI>(ln, xi, JxW, lam, mu, S, P);
                    SjShape H;
                    sj_shape(xi, eta, zeta, S.ih, H);
                    double ga[3];
                    sj_grad<a>(H, ga);
                    if constexpr (!PHI)
                      {
                        if (e == 7)
                          any_compressed = any_compressed || P.compressed;
                        // K[(a,c),(b,d)] += a_w ga_c gb_d + mu g_w ga_d gb_c + delta_cd mu g_w ga . gb
                        const double LA = P.aw * ga[COMP], mgw = mu * P.gw;
                        const double MA[3] = {mgw * ga[0], mgw * ga[1], mgw * ga[2]};
                        sj_for<8>([&](auto Bc) __attribute__((always_inline)) {
                          constexpr int b = decltype(Bc)::value, o = (ex + (b & 1)) + 3 * (ey + ((b >> 1) & 1)) + 9 * (ez + (b >> 2));
                          double gb[3];
                          sj_grad<b>(H, gb);
                          const double t = MA[0] * gb[0] + MA[1] * gb[1] + MA[2] * gb[2];
#pragma unroll
                          for (int d = 0; d < 3; ++d)
                            {
                              const double kv = LA * gb[d] + MA[d] * gb[COMP] + (d == COMP ? t : 0.0);
                              acc[o][d] += kv;
                              if (b == a && d == COMP)
                                dcell += kv;
                            }
                        });
                      }
                    else
                      {
                        // K[(a,phi),(b,d)] += Na (cpu sigma+_d . gb - cdiv gb_d);  K[(a,phi),(b,phi)] += cpp Na Nb + cgg ga . gb
                        const double Na = sj_value<a>(H);
                        const double cpu = P.cpu * Na, cdiv = P.cdiv * Na, cpp = P.cpp * Na;
                        const double W[3][3] = {{cpu * P.s00 - cdiv, cpu * P.s01, cpu * P.s02},
                                                {cpu * P.s01, cpu * P.s11 - cdiv, cpu * P.s12},
                                                {cpu * P.s02, cpu * P.s12, cpu * P.s22 - cdiv}};
                        const double GA[3] = {P.cgg * ga[0], P.cgg * ga[1], P.cgg * ga[2]};
                        sj_for<8>([&](auto Bc) __attribute__((always_inline)) {
                          constexpr int b = decltype(Bc)::value, o = (ex + (b & 1)) + 3 * (ey + ((b >> 1) & 1)) + 9 * (ez + (b >> 2));
                          double gb[3];
                          sj_grad<b>(H, gb);
                          const double Nb = sj_value<b>(H);
#pragma unroll
                          for (int d = 0; d < 3; ++d)
                            acc[o][d] += W[d][0] * gb[0] + W[d][1] * gb[1] + W[d][2] * gb[2];
                          const double kv = cpp * Nb + (GA[0] * gb[0] + GA[1] * gb[1] + GA[2] * gb[2]);
                          acc[o][3] += kv;
                          if (b == a)
                            dcell += kv;
                        });
                      }
                  }
              }
            const double dg = fabs(dcell);
            if (dg != 0.0)
              ph += dg;
            else
              need_avg |= 1u << e;
          }
      });

      if constexpr (COMP == 0)
        if (A.n_compressed)
          {
            const unsigned long long m = __ballot(any_compressed);
            if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
              atomicAdd(A.n_compressed, (int)__popcll(m));
          }

      // ---- the row goes out: constrained rows and eliminated columns as masks (cracks.cc:2440-2456), the placeholder on the
      // diagonal of a constrained row
      const long long off = v.nadj_ptr[row];
      const unsigned nmask = cv.nbr_mask[row];
      const int deg = __popc(nmask & 0x7ffffffu);
      sj_for<27>([&](auto Oc) __attribute__((always_inline)) {
        constexpr int o = decltype(Oc)::value, ox = o % 3, oy = (o / 3) % 3, oz = o / 9;
        if ((nmask >> o) & 1u)
          {
            int sl = __popc(nmask & ((1u << o) - 1u));
            if (nmask >> 31) // row not in lattice order: permutation of the ranks
              sl = cv.row_perm[off + sl];
            const int nb = sj_local_id(cv, gi + ox - 1, gj + oy - 1, gk + oz - 1);
            const unsigned nflag = nb >= 0 ? v.node_flags[nb] : 0u;
            double val[NC];
#pragma unroll
            for (int d = 0; d < NC; ++d)
              {
                val[d] = (rcon || ((nflag >> d) & 1u)) ? 0.0 : acc[o][d];
                if (o == 13 && d == COMP && rcon)
                  val[d] = ph;
              }
            if constexpr (NCOL == 4)
              {
                double *dst = A.vals_uu + 16 * off + (long long)COMP * 4 * deg + sl * 4;
                dst[0] = val[0], dst[1] = val[1], dst[2] = val[2];
                dst[3] = PHI ? val[NC - 1] : 0.0; // the structurally zero (u,phi) block (cracks.cc:2333-2337)
              }
            else if constexpr (PHI)
              {
                double *dst = A.vals_pu + 3 * off + sl * 3;
                dst[0] = val[0], dst[1] = val[1], dst[2] = val[2];
                A.vals_pp[off + sl] = val[NC - 1];
              }
            else
              {
                double *dst = A.vals_uu + 9 * off + (long long)COMP * 3 * deg + sl * 3;
                dst[0] = val[0], dst[1] = val[1], dst[2] = val[2];
                if (!cv.up_block_cleared) // (kernel-uniform) a kept (u,phi) block holds its zeros already
                  A.vals_up[3 * off + (long long)COMP * deg + sl] = 0.0;
              }
          }
      });

      // ---- rare: a constrained row next to a cell whose part of the diagonal vanished.  The diagonal is written again with
      // the complete placeholder, by the same lane behind its first store.
      if (rcon && need_avg != 0u)
        {
#pragma unroll 1
          for (int e = 0; e < 8; ++e)
            {
              const int ci = gi - 1 + (e & 1), cj = gj - 1 + ((e >> 1) & 1), ck = gk - 1 + (e >> 2);
              if (!((need_avg >> e) & 1u))
                continue;
              double lam = S.lam, mu = S.mu;
              if (cv.cell_lam)
                {
                  const long long cidx = ci + (long long)(cv.NX - 1) * (cj + (long long)(cv.NY - 1) * ck);
                  lam = cv.cell_lam[cidx];
                  mu = cv.cell_mu[cidx];
                }
              double U[6][8];
              sj_load_cell(v, cv, ci, cj, ck, U);
              ph += sj_cell_diag_mean(U, lam, mu, S);
            }
          int sl = __popc(nmask & ((1u << 13) - 1u));
          if (nmask >> 31)
            sl = cv.row_perm[off + sl];
          if constexpr (NCOL == 4)
            A.vals_uu[16 * off + (long long)COMP * 4 * deg + sl * 4 + COMP] = ph;
          else if constexpr (PHI)
            A.vals_pp[off + sl] = ph;
          else
            A.vals_uu[9 * off + (long long)COMP * 3 * deg + sl * 3 + COMP] = ph;
        }
    }

    // SPARSE: is the node a vertex of a cell whose byte k_cart_split3_mark set?  Cells outside the lattice read as 0.
    __device__ __forceinline__ bool sj_node_touched(const CartView &cv, const uint8_t *cell_comp, int gi, int gj, int gk)
    {
      bool any = false;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        {
          const int ci = gi - 1 + (e & 1), cj = gj - 1 + ((e >> 1) & 1), ck = gk - 1 + (e >> 2);
          if (ci >= 0 && ci < cv.NX - 1 && cj >= 0 && cj < cv.NY - 1 && ck >= 0 && ck < cv.NZ - 1)
            any = any || cell_comp[ci + (long long)(cv.NX - 1) * (cj + (long long)(cv.NY - 1) * ck)] != 0;
        }
      return any;
    }

    // k_cart_split3_mark (CartPlan::voldev_sparse): lane <-> lattice cell, over the cells that touch an owned row -- the cell
    // range [o0 - 1, o1] of the owned box, cut to the lattice.  tr E at the 27 q-points by the statements of the rows above
    // (sj_line_setup, sj_trace, split3::voldev: the sign is the same source statement on the same operands); only the
    // displacements enter.  One byte per cell: 1 = some q-point has h = 0.  Such a cell sets the flag of every tile-chunk of
    // grid[PFM_ZC_UU3] that holds one of its owned vertices (plain int stores of 1: order-independent) and is counted by the
    // rule of sj_row: the cell whose lowest vertex is a row of this rank, ballot + one integer atomic per wave.
    struct SmArgs
    {
      DevView v;
      CartView cv;
      double ih[3], lam, mu;
      uint8_t *cell_comp;
      int *tile_flag, *n_compressed;
      int c0[3], cn[3]; // first cell and cells per axis of the launch
      int ntx, nty, zc; // tile-chunks of grid[PFM_ZC_UU3]
    };
    // LEVEL: cv is a level lattice of a 3-D overlay.  A cell takes part only if all of its eight vertices exist on the level
    // (local_of_box >= 0: every cell of a regular row does); the owned vertices are the regular rows (row_of_box), and the
    // count is that of the level form of k_cart_split3_jac: the cell whose lowest vertex is a regular row of this rank.
    constexpr int SM_NT = 256;
    template <bool LEVEL>
    __global__ __launch_bounds__(SM_NT) void k_cart_split3_mark(SmArgs A)
    {
      const CartView &cv = A.cv;
      const long long id = (long long)blockIdx.x * SM_NT + threadIdx.x, n = (long long)A.cn[0] * A.cn[1] * A.cn[2];
      const bool in = id < n;
      bool compressed = false, counted = false;
      if (in)
        {
          const int ci = A.c0[0] + (int)(id % A.cn[0]), cj = A.c0[1] + (int)(id / A.cn[0] % A.cn[1]), ck = A.c0[2] + (int)(id / ((long long)A.cn[0] * A.cn[1]));
          const long long cidx = ci + (long long)(cv.NX - 1) * (cj + (long long)(cv.NY - 1) * ck);
          double lam = A.lam, mu = A.mu;
          if (cv.cell_lam)
            {
              lam = cv.cell_lam[cidx];
              mu = cv.cell_mu[cidx];
            }
          double U[6][8];
          bool whole = true;
#pragma unroll
          for (int b = 0; b < 8; ++b)
            {
              const int nd = sj_local_id(cv, ci + (b & 1), cj + ((b >> 1) & 1), ck + (b >> 2));
              const bool has = nd >= 0;
              whole = whole && has;
              U[0][b] = has ? A.v.u[0][nd] : 0.0;
              U[1][b] = has ? A.v.u[1][nd] : 0.0;
              U[2][b] = has ? A.v.u[2][nd] : 0.0;
              U[3][b] = U[4][b] = U[5][b] = 0.0; // (the phase fields do not enter the trace)
            }
#pragma unroll 1
          for (int p = 0; p < (LEVEL && !whole ? 0 : 9); ++p)
            {
              const double eta = sj_gx(p % 3), zeta = sj_gx(p / 3);
              SjLine ln;
              sj_line_setup(U, eta, zeta, A.ih, ln);
#pragma unroll 1
              for (int qx = 0; qx < 3; ++qx)
                {
                  double g00, g11, g22;
                  const double trE = sj_trace(ln, sj_gx(qx), g00, g11, g22);
                  const split3::VolDev V = split3::voldev(trE, lam, mu);
                  compressed = compressed || V.h == 0.0;
                }
            }
          A.cell_comp[cidx] = compressed ? 1 : 0;
          if (compressed)
            {
              const int nch_z = (cv.o1[2] - cv.o0[2] + A.zc) / A.zc;
#pragma unroll
              for (int b = 0; b < 8; ++b)
                {
                  const int i = ci + (b & 1) - cv.o0[0], j = cj + ((b >> 1) & 1) - cv.o0[1], k = ck + (b >> 2) - cv.o0[2];
                  if (i >= 0 && i <= cv.o1[0] - cv.o0[0] && j >= 0 && j <= cv.o1[1] - cv.o0[1] && k >= 0 && k <= cv.o1[2] - cv.o0[2] && k / A.zc < nch_z)
                    {
                      if constexpr (LEVEL)
                        {
                          const int row = cv.row_of_box[(ci + (b & 1)) + (long long)cv.NX * ((cj + ((b >> 1) & 1)) + (long long)cv.NY * (ck + (b >> 2)))];
                          if (row < 0 || row >= A.v.n_owned)
                            continue; // no row of this launch
                        }
                      A.tile_flag[i / T3X + A.ntx * (j / T3Y + A.nty * (k / A.zc))] = 1;
                    }
                }
              if (ci >= cv.o0[0] && ci <= cv.o1[0] && cj >= cv.o0[1] && cj <= cv.o1[1] && ck >= cv.o0[2] && ck <= cv.o1[2])
                {
                  const int row = LEVEL ? cv.row_of_box[ci + (long long)cv.NX * (cj + (long long)cv.NY * ck)] : sj_local_id(cv, ci, cj, ck);
                  counted = row >= 0 && row < A.v.n_owned;
                }
            }
        }
      const unsigned long long m = __ballot(counted);
      if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
        atomicAdd(A.n_compressed, (int)__popcll(m));
    }

    constexpr int SJ_NT = 64; // one wave: T3X x T3Y nodes of two planes
    static_assert(T3X * T3Y * 2 == SJ_NT, "two node planes of a k_cart_uu3 tile per wave");

    // LEVEL (CartPlan::voldev_jac under PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS / _ALL_LEVELS): cv is one refinement level's
    // lattice of a 3-D overlay (CartView::row_of_box) -- the rows of the launch are those of row_of_box (the statement of cart_row_id, pfm_cart_common.h), -1 = hanging, parent,
    // mixed-level or ghost node: not a row of this launch, the lane passes it by.  Everything else is the box form: nodes of
    // other levels inside the bounding box read as absent (local_of_box == -1) and only enter rows that are not written, a
    // row at a face of the domain has fewer cells and neighbours (nbr_mask, always with bit 31: row_perm), owned_lex is 0.
    template <int NCOL, bool LEVEL>
    __global__ __launch_bounds__(SJ_NT) void k_cart_split3_jac(SjArgs A)
    {
      const CartView &cv = A.cv;
      const int OWX = cv.o1[0] - cv.o0[0] + 1, OWY = cv.o1[1] - cv.o0[1] + 1, OWZ = cv.o1[2] - cv.o0[2] + 1;
      const int ntx = (OWX + T3X - 1) / T3X, nty = (OWY + T3Y - 1) / T3Y;
      const int zc = A.zc, nch = (OWZ + zc - 1) / zc;
      int bid = (int)((blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3)); // XCD-aware launch, pfm_internal.h
      const bool listed = cv.tile_sel == 2 && cv.bnd_uu3 != nullptr; // compact launch over the boundary tiles (zc == 1)
      if (listed)
        {
          if (bid >= cv.n_bnd_uu3)
            return;
          bid = cv.bnd_uu3[bid];
        }
      if (bid >= ntx * nty * nch)
        return; // padding of the XCD-aware grid
      const int tix = bid % ntx, tiy = (bid / ntx) % nty, chunk = bid / (ntx * nty);
      const int i0 = cv.o0[0] + tix * T3X, j0 = cv.o0[1] + tiy * T3Y;
      const int kA = cv.o0[2] + chunk * zc, kB = min(kA + zc, cv.o1[2] + 1); // node planes [kA, kB)
      if (!listed && cart_tile_skipped(cv, cart_range_has_ghost(cv, 0, i0 - 1, i0 + T3X) || cart_range_has_ghost(cv, 1, j0 - 1, j0 + T3Y) ||
                                               cart_range_has_ghost(cv, 2, kA - 1, kB)))
        return; // overlapped assembly: the other launch owns this tile
      const int t = threadIdx.x, gi = i0 + t % T3X, gj = j0 + (t / T3X) % T3Y;
      if (gi > cv.o1[0] || gj > cv.o1[1])
        return; // partial tile (no barrier anywhere: a lane may leave)
#pragma unroll 1
      for (int gk = kA + t / (T3X * T3Y); gk < kB; gk += 2)
        {
          const int row = LEVEL ? cv.row_of_box[gi + (long long)cv.NX * (gj + (long long)cv.NY * gk)] // a regular row of this level, or -1
                                : sj_local_id(cv, gi, gj, gk);                                       // an owned node of the box: its row
          if (row < 0 || row >= A.v.n_owned)
            continue;
          const unsigned row_flag = A.v.node_flags[row];
          sj_row<0, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<1, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<2, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<3, NCOL>(A, gi, gj, gk, row, row_flag);
        }
    }

    // SPARSE form (CartPlan::voldev_sparse, PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE / _ALL_SPARSE; LEVEL: on a level lattice,
    // PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE / _ALL_LEVELS_SPARSE, the rows of the launch are those of row_of_box as above), a
    // second template of the same name with an argument of its own: the unsplit kernels have written every row, and this
    // launch writes again the rows of the nodes that are a vertex of a cell with a compressed q-point (SjSparseArgs::cell_comp),
    // by the same sj_row calls -- the same bytes as the plain form.  A workgroup whose tile-chunk has no such node
    // (SjSparseArgs::tile_flag) returns at once, a lane passes every other node by.  It always runs whole (tile_sel 0: no
    // list of boundary tiles, no skipped tile).  The plain kernel above is left as it was, statement for statement: its four
    // instantiations are the parent's instruction for instruction, which sharing its body with this one did not give.
    template <int NCOL, bool LEVEL, bool SPARSE>
    __global__ __launch_bounds__(SJ_NT) void k_cart_split3_jac(SjArgs A, SjSparseArgs X)
    {
      static_assert(SPARSE, "the sparse form");
      const CartView &cv = A.cv;
      const int OWX = cv.o1[0] - cv.o0[0] + 1, OWY = cv.o1[1] - cv.o0[1] + 1, OWZ = cv.o1[2] - cv.o0[2] + 1;
      const int ntx = (OWX + T3X - 1) / T3X, nty = (OWY + T3Y - 1) / T3Y;
      const int zc = A.zc, nch = (OWZ + zc - 1) / zc;
      const int bid = (int)((blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3)); // XCD-aware launch, pfm_internal.h
      if (bid >= ntx * nty * nch)
        return; // padding of the XCD-aware grid
      if (X.tile_flag[bid] == 0)
        return; // no node of this tile-chunk touches a compressed cell: its rows stay the unsplit kernels'
      const int tix = bid % ntx, tiy = (bid / ntx) % nty, chunk = bid / (ntx * nty);
      const int i0 = cv.o0[0] + tix * T3X, j0 = cv.o0[1] + tiy * T3Y;
      const int kA = cv.o0[2] + chunk * zc, kB = min(kA + zc, cv.o1[2] + 1); // node planes [kA, kB)
      const int t = threadIdx.x, gi = i0 + t % T3X, gj = j0 + (t / T3X) % T3Y;
      if (gi > cv.o1[0] || gj > cv.o1[1])
        return; // partial tile (no barrier anywhere: a lane may leave)
#pragma unroll 1
      for (int gk = kA + t / (T3X * T3Y); gk < kB; gk += 2)
        {
          const int row = LEVEL ? cv.row_of_box[gi + (long long)cv.NX * (gj + (long long)cv.NY * gk)] // a regular row of this level, or -1
                                : sj_local_id(cv, gi, gj, gk);                                       // an owned node of the box: its row
          const bool touched = row >= 0 && row < A.v.n_owned && sj_node_touched(cv, X.cell_comp, gi, gj, gk);
          const unsigned long long m = __ballot(touched);
          if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
            atomicAdd(X.n_rows, (int)__popcll(m));
          if (!touched)
            continue;
          const unsigned row_flag = A.v.node_flags[row];
          sj_row<0, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<1, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<2, NCOL>(A, gi, gj, gk, row, row_flag);
          sj_row<3, NCOL>(A, gi, gj, gk, row, row_flag);
        }
    }
  } // namespace

  // The matrix values of pl = plan_cart(...) with CartPlan::voldev_jac: every block, whole (phase 0) or in the second half.
  // n_compressed (device, may be nullptr): zeroed by the caller; gets the number of cells with a compressed q-point.
  // sparse (CartPlan::voldev_sparse): the buffers k_cart_split3_mark has filled; the count is that kernel's.
  int launch_cart_split3_jac(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, double *const *d_values,
                             int *n_compressed, hipStream_t s, const SplitSparse *sparse)
  {
    if (!pl.split3_jac() || (pl.voldev_sparse != (sparse != nullptr)))
      return PFM_ERR_UNSUPPORTED;
    const TileGrid &g = pl.grid[PFM_ZC_UU3];
    if (g.n_tiles == 0)
      return PFM_OK;
    const bool il = pl.interleaved; // one block of values
    SjArgs ka{v, cv, make_sj_scal(p, cv), d_values[0], il ? nullptr : d_values[1], il ? nullptr : d_values[2], il ? nullptr : d_values[3],
              sparse ? nullptr : n_compressed, g.zc};
    const bool level = cv.row_of_box != nullptr;
    if (level && (!cv.nbr_mask || !cv.row_perm || cv.owned_lex))
      return PFM_ERR_INTERNAL; // (the overlay's row tables: ensure_overlay3_ready)
    using Kernel = void (*)(SjArgs);
    static const Kernel kernel[2][2] = {{k_cart_split3_jac<3, false>, k_cart_split3_jac<3, true>}, // by layout and LEVEL
                                        {k_cart_split3_jac<4, false>, k_cart_split3_jac<4, true>}};
    using SparseKernel = void (*)(SjArgs, SjSparseArgs);
    static const SparseKernel kernel_sparse[2][2] = {{k_cart_split3_jac<3, false, true>, k_cart_split3_jac<3, true, true>},
                                                     {k_cart_split3_jac<4, false, true>, k_cart_split3_jac<4, true, true>}};
    if (sparse)
      hipLaunchKernelGGL(kernel_sparse[il][level], dim3(xcd_grid(g.n_tiles)), dim3(SJ_NT), 0, s, ka, SjSparseArgs{sparse->cell_comp, sparse->tile_flag, sparse->n_rows});
    else
      hipLaunchKernelGGL(kernel[il][level], dim3(xcd_grid(g.n_tiles)), dim3(SJ_NT), 0, s, ka);
    return hipGetLastError() == hipSuccess ? PFM_OK : PFM_ERR_HIP;
  }

  // CartPlan::voldev_sparse, in front of the unsplit kernels: the cell bytes, the tile-chunk flags of pl.grid[PFM_ZC_UU3] and
  // the count of the compressed cells (all zeroed by the caller)
  int launch_cart_split3_mark(const CartPlan &pl, const DevView &v, const CartView &cv, const pfm_params &p, const SplitSparse &sparse,
                              int *n_compressed, hipStream_t s)
  {
    if (!pl.split3_jac() || !pl.voldev_sparse || !n_compressed)
      return PFM_ERR_UNSUPPORTED;
    const TileGrid &g = pl.grid[PFM_ZC_UU3];
    if (g.n_tiles == 0)
      return PFM_OK;
    const int N[3] = {cv.NX, cv.NY, cv.NZ};
    SmArgs ka{};
    ka.v = v, ka.cv = cv, ka.lam = p.lambda, ka.mu = p.mu;
    ka.cell_comp = sparse.cell_comp, ka.tile_flag = sparse.tile_flag, ka.n_compressed = n_compressed;
    ka.ntx = g.ntx, ka.nty = g.nty, ka.zc = g.zc;
    long long n = 1;
    for (int d = 0; d < 3; ++d)
      {
        ka.ih[d] = 1.0 / cv.h[d]; // (make_sj_scal's statement)
        ka.c0[d] = std::max(cv.o0[d] - 1, 0);
        ka.cn[d] = std::min(cv.o1[d], N[d] - 2) - ka.c0[d] + 1;
        if (ka.cn[d] <= 0)
          return PFM_OK; // no cell
        n *= ka.cn[d];
      }
    hipLaunchKernelGGL(cv.row_of_box ? k_cart_split3_mark<true> : k_cart_split3_mark<false>, dim3((unsigned)((n + SM_NT - 1) / SM_NT)), dim3(SM_NT), 0, s, ka);
    return hipGetLastError() == hipSuccess ? PFM_OK : PFM_ERR_HIP;
  }
} // namespace pfm

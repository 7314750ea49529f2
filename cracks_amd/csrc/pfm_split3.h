// pfm_split3.h — spectral tension / compression split of the stress in 3-D (PFM_SPLIT_SPECTRAL), used by the
// 3-D SPLIT instantiations of the general cell kernel (pfm_kernels.hip).  The reference has no 3-D split (its closed form
// reads the 2 x 2 corner of the strain, cracks.cc:1683-1690); the law is fixed in cracks_amd/split3d.py, which is the numpy
// statement of what stands here:
//
//   E = sum_i l_i n_i n_i^T,  h(x) = 0 if x < 0 else 1   (zero counts as tension, cracks.cc:2068-2101)
//   E+ = sum_i max(l_i, 0) n_i n_i^T,  tr+ = max(tr E, 0)
//   sigma+ = lambda tr+ I + 2 mu E+,   sigma- = lambda (tr E - tr+) I + 2 mu (E - E+)
//   dE+[H] = sum_i h(l_i) (n_i^T H n_i) n_i n_i^T + sum_{i != j} theta_ij (n_i^T H n_j) n_i n_j^T
//   theta_ij = (max(l_i, 0) - max(l_j, 0)) / (l_i - l_j),  = h(l_i) when l_i == l_j in floating point
//
// At the end of the file: the volumetric-deviatoric split (PFM_SPLIT_VOLDEV), which needs none of the above.
//
// Plain C++ without hardware estimates: the same statements compile for the device and, alone, for the CPU
// (tests/cpp/split3_main.cpp).  Voigt order 00, 11, 22, 01, 02, 12; a direction H enters with its shears DOUBLED (the
// columns of B_b in the kernel are engineering strains), a stress leaves with plain components: the tangents are symmetric.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFM_HD __host__ __device__ inline
#else
#define PFM_HD inline
#endif

namespace pfm
{
  namespace split3
  {
    // Voigt index -> tensor indices
    PFM_HD constexpr int vi(int r) { return r < 3 ? r : (r == 5 ? 1 : 0); }
    PFM_HD constexpr int vj(int r) { return r < 3 ? r : (r == 3 ? 1 : 2); }
    // packed upper triangle of a symmetric 6 x 6: entry (r, k), r <= k
    PFM_HD constexpr int tri(int r, int k) { return r * 6 - r * (r - 1) / 2 + (k - r); }
    PFM_HD constexpr int sym(int r, int k) { return r <= k ? tri(r, k) : tri(k, r); }

    // Cyclic Jacobi on a symmetric 3 x 3 tensor A (Voigt, plain components): eigenvalues l, eigenvectors the COLUMNS of
    // N.  A rotation is skipped when its off-diagonal entry is exactly zero -- a diagonal tensor returns its diagonal and
    // the identity untouched -- and an entry below 2^-60 of its two diagonals is dropped (eigenvalue error far below an
    // ulp of |A|).  Ten sweeps bound the loop; 3 x 3 tensors converge quadratically and take four or five.  Every divisor
    // is either non-zero by the test in front of it or at least 1.
    PFM_HD void eigen_sym3(const double A[6], double l[3], double N[3][3])
    {
      double a[3][3] = {{A[0], A[3], A[4]}, {A[3], A[1], A[5]}, {A[4], A[5], A[2]}};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          N[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
      for (int sweep = 0; sweep < 10; ++sweep)
        {
          if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0)
            break;
#pragma unroll
          for (int r = 3; r < 6; ++r)
            {
              const int p = vi(r), q = vj(r), o = 3 - p - q;
              const double apq = a[p][q];
              if (apq == 0.0)
                continue;
              if (fabs(apq) <= 0x1p-60 * (fabs(a[p][p]) + fabs(a[q][q])))
                {
                  a[p][q] = a[q][p] = 0.0;
                  continue;
                }
              // tan of the rotation angle: the smaller root of t^2 + 2 t theta - 1 = 0 (|t| <= 1); theta may overflow to
              // +-inf (t = 0 then)
              const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
              const double at = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
              const double t = theta < 0.0 ? -at : at;
              const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
              a[p][p] -= t * apq;
              a[q][q] += t * apq;
              a[p][q] = a[q][p] = 0.0;
              const double aop = a[o][p], aoq = a[o][q];
              a[o][p] = a[p][o] = cs * aop - sn * aoq;
              a[o][q] = a[q][o] = sn * aop + cs * aoq;
#pragma unroll
              for (int i = 0; i < 3; ++i)
                {
                  const double np = N[i][p], nq = N[i][q];
                  N[i][p] = cs * np - sn * nq;
                  N[i][q] = sn * np + cs * nq;
                }
            }
        }
      l[0] = a[0][0];
      l[1] = a[1][1];
      l[2] = a[2][2];
    }

    struct Split3
    {
      double Ep[6];  // E+ (Voigt, plain components)
      double Pp[21]; // dE+/dE, packed upper triangle (tri), columns for doubled shears
      double htr;    // h(tr E)
    };

    // E (Voigt, plain components) -> E+ and, TANGENT, its derivative
    template <bool TANGENT>
    PFM_HD void split_strain(const double E[6], Split3 &S)
    {
      double l[3], N[3][3];
      eigen_sym3(E, l, N);
      const double lp[3] = {fmax(l[0], 0.0), fmax(l[1], 0.0), fmax(l[2], 0.0)};
#pragma unroll
      for (int r = 0; r < 6; ++r)
        {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < 3; ++i)
            s += lp[i] * N[vi(r)][i] * N[vj(r)][i];
          S.Ep[r] = s;
        }
      S.htr = (E[0] + E[1] + E[2]) < 0.0 ? 0.0 : 1.0;
      if (TANGENT)
        {
#pragma unroll
          for (int e = 0; e < 21; ++e)
            S.Pp[e] = 0.0;
          // the six dyads sym(n_i n_j^T), i <= j, with their weights h(l_i) and 2 theta_ij
#pragma unroll
          for (int d = 0; d < 6; ++d)
            {
              const int i = vi(d), j = vj(d);
              double w;
              if (i == j)
                w = l[i] < 0.0 ? 0.0 : 1.0;
              else
                {
                  const double gap = l[i] - l[j];
                  w = 2.0 * (gap == 0.0 ? (l[i] < 0.0 ? 0.0 : 1.0) : (lp[i] - lp[j]) / gap);
                }
              double m[6];
#pragma unroll
              for (int r = 0; r < 6; ++r)
                m[r] = 0.5 * (N[vi(r)][i] * N[vj(r)][j] + N[vj(r)][i] * N[vi(r)][j]);
#pragma unroll
              for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int k = r; k < 6; ++k)
                  S.Pp[tri(r, k)] += (w * m[r]) * m[k];
            }
        }
    }

    // sigma+ and sigma- (Voigt, plain components) of a split strain
    PFM_HD void split_stress3(const double E[6], const Split3 &S, double lam, double mu, double sp[6], double sm[6])
    {
      const double trE = E[0] + E[1] + E[2], trp = fmax(trE, 0.0);
#pragma unroll
      for (int r = 0; r < 6; ++r)
        {
          const double id = r < 3 ? 1.0 : 0.0;
          sp[r] = lam * trp * id + 2 * mu * S.Ep[r];
          sm[r] = lam * (trE - trp) * id + 2 * mu * (E[r] - S.Ep[r]);
        }
    }

    // C+ = d sigma+ / dE and C- = d sigma- / dE, packed upper triangles
    PFM_HD void split_tangent3(const Split3 &S, double lam, double mu, double Cp[21], double Cm[21])
    {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = r; k < 6; ++k)
          {
            const double one = (r < 3 && k < 3) ? 1.0 : 0.0;           // I (x) I
            const double ids = r == k ? (r < 3 ? 1.0 : 0.5) : 0.0;     // symmetric identity, doubled-shear columns
            const double P = S.Pp[tri(r, k)];
            Cp[tri(r, k)] = lam * S.htr * one + 2 * mu * P;
            Cm[tri(r, k)] = lam * (1.0 - S.htr) * one + 2 * mu * (ids - P);
          }
    }

    // ---- volumetric-deviatoric split (PFM_SPLIT_VOLDEV; cracks_amd/split3d.py: voldev_split, voldev_tangent)
    //
    //   K = lambda + 2 mu / 3,  tr+ = max(tr E, 0),  tr- = tr E - tr+,  h = h(tr E)
    //   sigma+ = K tr+ I + 2 mu (E - (tr E / 3) I)            sigma- = K tr- I
    //   C+ = K h I (x) I + 2 mu (I_s - 1/3 I (x) I)           C- = K (1 - h) I (x) I
    //
    // No eigenpairs: sigma+ = sp_iso I + 2 mu E, sigma- = sm_iso I, and g C+ + d_mat C- = a I (x) I + 2 (mu g) I_s is the
    // tangent of an isotropic material (voldev_tangent_a).  Finite for finite input; no division but the constant 1/3.
    struct VolDev
    {
      double sp_iso; // K tr+ - (2 mu / 3) tr E
      double sm_iso; // K tr-
      double h;      // h(tr E)
    };

    PFM_HD VolDev voldev(double trE, double lam, double mu)
    {
      const double K = lam + 2.0 * mu / 3.0, trp = fmax(trE, 0.0);
      VolDev S;
      S.sp_iso = K * trp - (2.0 * mu / 3.0) * trE;
      S.sm_iso = K * (trE - trp);
      S.h = trE < 0.0 ? 0.0 : 1.0;
      return S;
    }

    // a of  g C+ + d_mat C- = a I (x) I + 2 b I_s,  b = mu g
    PFM_HD double voldev_tangent_a(const VolDev &S, double lam, double mu, double g, double d_mat)
    {
      return lam * (g * S.h + d_mat * (1.0 - S.h)) - (2.0 * mu / 3.0) * (1.0 - S.h) * (g - d_mat);
    }

    // one component of sigma+ = sp_iso I + 2 mu E: e the component of E, diag whether it sits on the diagonal.  The kernel
    // and voldev_stress3 both form sigma+ through this statement, and sigma- as sm_iso on the diagonal.
    PFM_HD double voldev_sigma_plus(const VolDev &S, double mu, double e, bool diag) { return (diag ? S.sp_iso : 0.0) + 2 * mu * e; }

    // sigma+ and sigma- (Voigt, plain components)
    PFM_HD void voldev_stress3(const double E[6], double lam, double mu, double sp[6], double sm[6])
    {
      const VolDev S = voldev(E[0] + E[1] + E[2], lam, mu);
#pragma unroll
      for (int r = 0; r < 6; ++r)
        {
          sp[r] = voldev_sigma_plus(S, mu, E[r], r < 3);
          sm[r] = r < 3 ? S.sm_iso : 0.0;
        }
    }

    // C+ and C-, packed upper triangles in the form of split_tangent3: g = 1, d_mat = 0 is C+, g = 0, d_mat = 1 is C-.
    // (For the host program and as documentation: the kernel keeps only voldev_tangent_a and b = mu g per q-point.)
    PFM_HD void voldev_tangent3(const double E[6], double lam, double mu, double Cp[21], double Cm[21])
    {
      const VolDev S = voldev(E[0] + E[1] + E[2], lam, mu);
      const double ap = voldev_tangent_a(S, lam, mu, 1.0, 0.0), am = voldev_tangent_a(S, lam, mu, 0.0, 1.0);
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = r; k < 6; ++k)
          {
            const double one = (r < 3 && k < 3) ? 1.0 : 0.0;       // I (x) I
            const double ids = r == k ? (r < 3 ? 1.0 : 0.5) : 0.0; // symmetric identity, doubled-shear columns
            Cp[tri(r, k)] = ap * one + 2 * mu * ids;
            Cm[tri(r, k)] = am * one;
          }
    }
  } // namespace split3
} // namespace pfm

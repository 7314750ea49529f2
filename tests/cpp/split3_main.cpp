// Stand-alone host program for cracks_amd/csrc/pfm_split3.h (tests/test_split3d_host.py builds it host-only under
// AddressSanitizer and UBSan and compares what it prints with cracks_amd/split3d.py).  One line per tensor:
//   case <name> lam mu | E (6, Voigt) | sigma+ (6) | sigma- (6) | C+ (21) | C- (21)
// every number as a hexadecimal float (exact).  It also checks the header's own promises: finite output, an exactly
// diagonal tensor returns its diagonal and the identity, E = 0 gives theta = 1.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pfm_split3.h"

using namespace pfm::split3;

static int n_fail = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() // uniform in (-1, 1), splitmix64
{
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-52 - 1.0;
}

static void run(const char *name, const double E[6], double lam, double mu)
{
  Split3 S;
  split_strain<true>(E, S);
  double sp[6], sm[6], Cp[21], Cm[21];
  split_stress3(E, S, lam, mu, sp, sm);
  split_tangent3(S, lam, mu, Cp, Cm);
  // the residual-only form must give the same E+
  Split3 S0;
  split_strain<false>(E, S0);
  for (int r = 0; r < 6; ++r)
    if (S0.Ep[r] != S.Ep[r])
      {
        std::printf("FAIL %s: E+ differs between the two forms\n", name);
        ++n_fail;
      }
  std::printf("case %s %a %a |", name, lam, mu);
  for (int r = 0; r < 6; ++r)
    std::printf(" %a", E[r]);
  std::printf(" |");
  for (int r = 0; r < 6; ++r)
    std::printf(" %a", sp[r]);
  std::printf(" |");
  for (int r = 0; r < 6; ++r)
    std::printf(" %a", sm[r]);
  std::printf(" |");
  for (int e = 0; e < 21; ++e)
    std::printf(" %a", Cp[e]);
  std::printf(" |");
  for (int e = 0; e < 21; ++e)
    std::printf(" %a", Cm[e]);
  std::printf("\n");
  bool finite = true;
  for (int r = 0; r < 6; ++r)
    finite = finite && std::isfinite(sp[r]) && std::isfinite(sm[r]);
  for (int e = 0; e < 21; ++e)
    finite = finite && std::isfinite(Cp[e]) && std::isfinite(Cm[e]);
  if (!finite)
    {
      std::printf("FAIL %s: non-finite output\n", name);
      ++n_fail;
    }
}

// R diag(d) R^T for the rotation by angles (a, b, c) about z, y, x
static void rotated(const double d[3], double a, double b, double c, double E[6])
{
  const double Rz[3][3] = {{std::cos(a), -std::sin(a), 0}, {std::sin(a), std::cos(a), 0}, {0, 0, 1}};
  const double Ry[3][3] = {{std::cos(b), 0, std::sin(b)}, {0, 1, 0}, {-std::sin(b), 0, std::cos(b)}};
  const double Rx[3][3] = {{1, 0, 0}, {0, std::cos(c), -std::sin(c)}, {0, std::sin(c), std::cos(c)}};
  double T[3][3] = {}, R[3][3] = {};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k)
        T[i][j] += Rz[i][k] * Ry[k][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k)
        R[i][j] += T[i][k] * Rx[k][j];
  for (int r = 0; r < 6; ++r)
    {
      double s = 0.0;
      for (int k = 0; k < 3; ++k)
        s += R[vi(r)][k] * d[k] * R[vj(r)][k];
      E[r] = s;
    }
}

int main()
{
  const double lam = 121.15, mu = 80.77;
  char name[64];
  // mixed-sign random tensors, magnitudes 1e-8 ... 1e4
  const double mags[7] = {1e-8, 1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4};
  for (int m = 0; m < 7; ++m)
    for (int k = 0; k < 6; ++k)
      {
        double E[6];
        for (int r = 0; r < 6; ++r)
          E[r] = mags[m] * rnd();
        std::snprintf(name, sizeof name, "random_%d_%d", m, k);
        run(name, E, lam, k % 2 ? mu : 0.5 * mu);
      }
  // rotated tensors with prescribed eigenvalues of both signs
  const double spectra[5][3] = {{1.0, -0.5, 0.25}, {-1.0, -2.0, 3.0}, {0.3, 0.2, -0.7}, {-0.1, -0.2, -0.3}, {0.1, 0.2, 0.3}};
  for (int s = 0; s < 5; ++s)
    for (int k = 0; k < 3; ++k)
      {
        double E[6];
        rotated(spectra[s], 0.3 + 0.7 * k, -0.4 + 0.5 * k, 1.1 - 0.3 * k, E);
        std::snprintf(name, sizeof name, "rotated_%d_%d", s, k);
        run(name, E, lam, mu);
      }
  // repeated eigenvalues, rotated and exact
  const double rep[6][3] = {{2.0, 2.0, -1.0}, {-2.0, -2.0, 1.0}, {0.5, -3.0, -3.0}, {1.5, 1.5, 1.5}, {-1.5, -1.5, -1.5}, {0.25, 0.25, 0.75}};
  for (int s = 0; s < 6; ++s)
    {
      double E[6];
      rotated(rep[s], 0.9, 0.35, -0.6, E);
      std::snprintf(name, sizeof name, "repeated_rot_%d", s);
      run(name, E, lam, mu);
      const double D[6] = {rep[s][0], rep[s][1], rep[s][2], 0.0, 0.0, 0.0};
      std::snprintf(name, sizeof name, "repeated_diag_%d", s);
      run(name, D, lam, mu);
    }
  // exactly diagonal, distinct entries; zero
  const double diags[4][6] = {{1.0, -2.0, 3.0, 0, 0, 0}, {-1e-8, 2e-8, 0.0, 0, 0, 0}, {1e4, -1e4, 5e3, 0, 0, 0}, {0.0, 0.0, -1.0, 0, 0, 0}};
  for (int s = 0; s < 4; ++s)
    {
      std::snprintf(name, sizeof name, "diagonal_%d", s);
      run(name, diags[s], lam, mu);
      double l[3], N[3][3];
      eigen_sym3(diags[s], l, N);
      bool ok = l[0] == diags[s][0] && l[1] == diags[s][1] && l[2] == diags[s][2];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          ok = ok && N[i][j] == (i == j ? 1.0 : 0.0);
      if (!ok)
        {
          std::printf("FAIL diagonal_%d: rotated\n", s);
          ++n_fail;
        }
    }
  {
    const double Z[6] = {0, 0, 0, 0, 0, 0};
    run("zero", Z, lam, mu);
    Split3 S;
    split_strain<true>(Z, S);
    // theta = 1 everywhere: dE+/dE is the symmetric identity
    for (int r = 0; r < 6; ++r)
      for (int k = r; k < 6; ++k)
        if (S.Pp[tri(r, k)] != (r == k ? (r < 3 ? 1.0 : 0.5) : 0.0))
          {
            std::printf("FAIL zero: dE+/dE (%d, %d) = %a\n", r, k, S.Pp[tri(r, k)]);
            ++n_fail;
          }
  }
  std::printf(n_fail ? "split3: FAILED\n" : "split3: OK\n");
  return n_fail ? 1 : 0;
}

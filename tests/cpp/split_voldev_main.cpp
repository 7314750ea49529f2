// Stand-alone host program for the volumetric-deviatoric law of cracks_amd/csrc/pfm_split3.h (tests/test_split_voldev_host.py
// builds it host-only under AddressSanitizer and UBSan and compares what it prints with cracks_amd/split3d.py).  One line
// per tensor:
//   case <name> lam mu g d_mat | E (6, Voigt) | sigma+ (6) | sigma- (6) | C+ (21) | C- (21) | a b
// every number as a hexadecimal float (exact); a, b: the two coefficients of g C+ + d_mat C- = a I (x) I + 2 b I_s that the
// kernel keeps per q-point.  It also checks the header's own promises: finite output, h(0) = 1, sigma- = 0 and C- = 0 for
// tr E >= 0, a I (x) I + 2 b I_s equal to g C+ + d_mat C- entry by entry.
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

static void fail(const char *name, const char *what)
{
  std::printf("FAIL %s: %s\n", name, what);
  ++n_fail;
}

static void run(const char *name, const double E[6], double lam, double mu, double g, double d_mat)
{
  double sp[6], sm[6], Cp[21], Cm[21];
  voldev_stress3(E, lam, mu, sp, sm);
  voldev_tangent3(E, lam, mu, Cp, Cm);
  const double trE = E[0] + E[1] + E[2];
  const VolDev S = voldev(trE, lam, mu);
  const double a = voldev_tangent_a(S, lam, mu, g, d_mat), b = mu * g;
  std::printf("case %s %a %a %a %a |", name, lam, mu, g, d_mat);
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
  std::printf(" | %a %a\n", a, b);
  bool finite = std::isfinite(a) && std::isfinite(b);
  for (int r = 0; r < 6; ++r)
    finite = finite && std::isfinite(sp[r]) && std::isfinite(sm[r]);
  for (int e = 0; e < 21; ++e)
    finite = finite && std::isfinite(Cp[e]) && std::isfinite(Cm[e]);
  if (!finite)
    fail(name, "non-finite output");
  if (S.h != (trE < 0.0 ? 0.0 : 1.0))
    fail(name, "h(tr E)");
  if (!(trE < 0.0))
    {
      bool zero = true;
      for (int r = 0; r < 6; ++r)
        zero = zero && sm[r] == 0.0;
      for (int e = 0; e < 21; ++e)
        zero = zero && Cm[e] == 0.0;
      if (!zero)
        fail(name, "sigma- or C- not zero for tr E >= 0");
    }
  // the isotropic pair against the two tangents, entry by entry (rounding of a handful of operations on the moduli)
  for (int r = 0; r < 6; ++r)
    for (int k = r; k < 6; ++k)
      {
        const double iso = ((r < 3 && k < 3) ? a : 0.0) + (r == k ? (r < 3 ? 2.0 * b : b) : 0.0);
        const double D = g * Cp[tri(r, k)] + d_mat * Cm[tri(r, k)];
        if (std::fabs(iso - D) > 0x1p-46 * (lam + 2.0 * mu))
          fail(name, "a I(x)I + 2 b I_s differs from g C+ + d_mat C-");
      }
}

int main()
{
  const double lam = 121.15, mu = 80.77;
  char name[64];
  // random tensors of magnitude 1e-8 ... 1e4, shifted so that tr E takes both signs
  const double mags[7] = {1e-8, 1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4};
  int n_pos = 0, n_neg = 0;
  for (int m = 0; m < 7; ++m)
    for (int k = 0; k < 8; ++k)
      {
        double E[6];
        const double shift = rnd();
        for (int r = 0; r < 6; ++r)
          E[r] = mags[m] * (rnd() + (r < 3 ? shift : 0.0));
        (E[0] + E[1] + E[2] < 0.0 ? n_neg : n_pos) += 1;
        std::snprintf(name, sizeof name, "random_%d_%d", m, k);
        run(name, E, lam, k % 2 ? mu : 0.5 * mu, 0.25 + 0.1 * k, k % 3 ? 1.0 : 0.5);
      }
  if (n_pos < 14 || n_neg < 14)
    fail("random", "the traces do not take both signs");
  // tr E exactly zero: traceless diagonals of exact binary fractions, pure shears, zero -- at every magnitude
  for (int m = 0; m < 7; ++m)
    {
      const double s = std::ldexp(1.0, (int)std::floor(std::log2(mags[m])));
      const double T[3][6] = {{0.5 * s, -0.25 * s, -0.25 * s, 0.3 * s, 0, 0}, {0, 0, 0, s, -0.5 * s, 0.25 * s}, {-s, 0.5 * s, 0.5 * s, 0, 0, 0.7 * s}};
      for (int k = 0; k < 3; ++k)
        {
          if (T[k][0] + T[k][1] + T[k][2] != 0.0)
            fail("traceless", "the trace is not exactly zero");
          std::snprintf(name, sizeof name, "traceless_%d_%d", m, k);
          run(name, T[k], lam, mu, 0.6, 1.0);
        }
    }
  {
    const double Z[6] = {0, 0, 0, 0, 0, 0};
    run("zero", Z, lam, mu, 0.6, 1.0);
    const VolDev S = voldev(0.0, lam, mu);
    if (S.h != 1.0 || S.sp_iso != 0.0 || S.sm_iso != 0.0)
      fail("zero", "h(0) = 1 and zero stresses");
  }
  // pure compression and pure dilation
  for (int m = 0; m < 7; ++m)
    for (int sgn = -1; sgn <= 1; sgn += 2)
      {
        const double a = sgn * mags[m], D[6] = {a, a, a, 0, 0, 0};
        std::snprintf(name, sizeof name, "isotropic_%d_%d", m, sgn < 0 ? 0 : 1);
        run(name, D, lam, mu, 0.6, sgn < 0 ? 0.0 : 1.0);
      }
  std::printf(n_fail ? "split_voldev: FAILED\n" : "split_voldev: OK\n");
  return n_fail ? 1 : 0;
}

// pfm_switches.h -- every PFM_* environment variable the library reads (pfm_delta_host.h, compiled alone, keeps its own
// reader of PFM_HOST_THREADS), each with what it selects.  Members: read once per process.  Static functions: read when
// called -- per call where the tests compare the variants in one process, else once per pfm_ctx_create.  No HIP include.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace pfm
{
  struct Switches
  {
    static bool set(const char *name) { return std::getenv(name) != nullptr; }
    static long long number(const char *name, long long unset) { return set(name) ? std::atoll(std::getenv(name)) : unset; }
    // ---- once per process
    const bool jac_sequential = set("PFM_JAC_SEQUENTIAL");         // 3-D box: the two Jacobian kernels in turn, not side by side
    const bool general_sequential = set("PFM_GENERAL_SEQUENTIAL"); // general family: the atomic class behind the colour classes
    const bool res_kernel = set("PFM_RES_KERNEL");                 // 3-D box Jacobian: the quadrature residual kernel runs as well
    const bool no_prio = set("PFM_NO_PRIO");                       // k_cart_phi4 without its wave priorities
    const bool uu_clock = set("PFM_UU_CLK");                       // phase clock of k_cart_uu3 (profiling; pfm_kernel_clock.h)
    const int phi_clock = !set("PFM_PHI_CLK") ? 0 : number("PFM_PHI_CLK", 0) == 2 ? 2 : 1; // ... of k_cart_phi4: 2 per role, else per phase
    // forced z-chunk lengths by PFM_ZC_*: k_cart_uu3, k_cart_phi4, k_cart_residual3*, k_cart_residual2m (0: the model's)
    const int zc[4] = {(int)number("PFM_UU_ZC", 0), (int)number("PFM_PHI_ZC", 0), (int)number("PFM_RES_ZC", 0), (int)number("PFM_RES2_ZC", 0)};
    const int host_threads = set("PFM_HOST_THREADS") ? std::max(1, (int)number("PFM_HOST_THREADS", 0)) : 0; // of the context build (0: unset)
    const char *const abort_trace = std::getenv("PFM_ABORT_TRACE"); // file that takes a backtrace of SIGABRT / SIGSEGV
    // ---- per call
    static bool side_stream() { return set("PFM_SIDE_STREAM"); }             // 3-D box Jacobian: the residual launch on the side stream
    static bool cart2d_one_launch() { return set("PFM_CART2D_ONE_LAUNCH"); } // k_cart2d_cells: one launch for both row groups
    // the (u,phi) block of a blocked 2-D box by a fill in front of the kernels (PFM_CART2D_NO_FILL: written with the rows)
    static bool cart2d_fill() { return !set("PFM_CART2D_NO_FILL") && !cart2d_one_launch(); }
    // a kept (u,phi) block (pfm_values_keep_up_block) is left alone (PFM_NO_KEEP_UP_BLOCK: the promise is ignored, every path writes it)
    static bool keep_up_block() { return !set("PFM_NO_KEEP_UP_BLOCK"); }
    // a kept (u,u) block (pfm_values_keep_uu_block) is left alone while it is current (PFM_NO_KEEP_UU_BLOCK: the promise is ignored, every assembly writes it)
    static bool keep_uu_block() { return !set("PFM_NO_KEEP_UU_BLOCK"); }
    static bool fused_scatter() { return !set("PFM_NO_FUSED_SCATTER"); }     // line search: the residual kernel scatters the solution
    static bool levels_concurrent() { return set("PFM_OVERLAY3_CONCURRENT"); } // 3-D overlay: a stream per level lattice
    static bool res_no_transfers() { return set("PFM_RES_NO_TRANSFERS"); }   // k_cart_residual3 instead of 3x / 3d
    static bool res_no_wide_transfers() { return set("PFM_RES_NO_WIDE_TRANSFERS"); } // k_cart_residual3d instead of 3x
    // ---- per pfm_ctx_create
    static bool no_patch() { return set("PFM_NO_PATCH"); }                   // no cartesian overlay: the general family alone
    static bool hanging_coloured() { return set("PFM_HANGING_COLOURED"); }   // 3-D hanging cells in plain colour classes
    static bool hanging_atomic() { return set("PFM_HANGING_ATOMIC"); }       // 3-D hanging cells in the class with FP64 atomics
    static long long overlay3_min_rows() { return number("PFM_OVERLAY3_MIN_ROWS", 64); }            // smallest level lattice kept
    static long long overlay3_max_table() { return number("PFM_OVERLAY3_MAX_TABLE", 400000000LL); } // largest lattice table kept
    static bool ctx_timing() { return set("PFM_CTX_TIMING"); }               // the phases of pfm_ctx_create on stderr
  };
  inline const Switches &switches()
  {
    static const Switches s;
    return s;
  }
} // namespace pfm

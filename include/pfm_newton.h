/* pfm_newton.h — C ABI of the other per-iteration sweeps of the reference's Newton / active-set loop
 * (SURVEY.md §8(f) N2, N3).  They share the context (mesh tables, node state, constraint flags) of
 * pfm_assemble.h, so that between two assemblies residual_total, diag_mass and the solution stay on the
 * device.  Same conventions: plain pointers and sizes, int status (pfm_status), pfm_last_error() for text.
 *
 * Reference interfaces replaced (all private members of FracturePhaseFieldProblem<dim>, cracks.cc):
 *   assemble_diag_mass_matrix()                       cracks.cc:2514-2562   -> pfm_diag_mass_device
 *   active-set block of newton_active_set()           cracks.cc:2826-2909   -> pfm_active_set_device
 *   the same block on a rank with ghost peers         cracks.cc:2826-2890, 2788 -> pfm_active_set_exchange
 *   compute_energy(), compute_tcv()                   cracks.cc:3615-3701, 3553-3611 -> pfm_functionals
 *   constraints_update.set_zero(residual); residual.l2_norm() / linfty_norm()
 *                                                     cracks.cc:2791-2794, 2918-2919, 2947-2949 -> pfm_residual_norms
 *   refinement indicator + level limit of refine_mesh() cracks.cc:3902-4116 -> pfm_refine_flags
 *   SolutionTransfer::interpolate                     cracks.cc:4137-4159   -> pfm_state_transfer
 *   min_cell_diameter                                 cracks.cc:3824-3835   -> pfm_min_cell_diameter
 *   compute_cod_array()                               cracks.cc:3337-3449   -> pfm_cod_buckets
 *   compute_point_stress(), compute_point_value()     cracks.cc:3285-3320, 3264-3283 -> pfm_point_eval
 */
#ifndef PFM_NEWTON_H
#define PFM_NEWTON_H

#include <stdint.h>

#include "pfm_assemble.h"

#ifdef __cplusplus
extern "C" {
#endif

/* diag_mass (cracks.cc:2514-2562): lumped (QGaussLobatto(2)) phase-field mass of every owned node,
 * d_mass[n_owned_nodes] (device pointer), asynchronous on the context's stream.  Displacement dofs have no
 * entry (the reference leaves them 0 and never reads them). */
int pfm_diag_mass_device(pfm_ctx *ctx, double *d_mass);

/* Active-set update (cracks.cc:2837-2886) + cycle counter (cracks.cc:2903-2909) + re-distribution of the
 * hanging nodes (cracks.cc:2888-2890), for the owned nodes of this rank:
 *   a phase-field dof that is not hanging becomes ACTIVE unless
 *        residual_total/diag_mass + c (phi - phi_old) <= 0  and  cycle_counter < 5;
 *   rounding: the criterion is fl(fl(residual_total / diag_mass) + fl(c fl(phi - phi_old))) in double, every operation
 *   rounded on its own (no fused multiply-add), as the reference and an unfused host statement evaluate it, so that
 *   the decisions agree at ties, -0.0 and NaN (NaN: active) included;
 *   an active dof gets phi := phi_old and a homogeneous constraint line (bit `dim` of the node's flag byte in
 *   the context, i.e. exactly what pfm_set_constraints would have been given); a dof that leaves the set
 *   increments its cycle counter.
 * d_residual_total, d_solution, d_old_solution: device vectors over the owned dofs in the context's layout
 * (d_solution is modified); d_mass from pfm_diag_mass_device; d_cycle_counter[n_owned_nodes] int32, zeroed by
 * the caller at the start of newton_active_set (cracks.cc:2811).
 * counts[0] = owned active dofs, counts[1] = cycling dofs among them, counts[2] = 1 if the set changed.
 * Synchronous (the counts are returned on the host, as the reference prints them).  On a partitioned mesh the
 * flags of ghost nodes are the caller's to exchange (pfm_get_constraints / pfm_set_constraints, or on the device
 * pfm_halo_exchange_flags; with hanging nodes: pfm_active_set_exchange). */
int pfm_active_set_device(pfm_ctx *ctx, const double *d_residual_total, const double *d_mass, double c,
                          double *d_solution, const double *d_old_solution, int32_t *d_cycle_counter,
                          int64_t counts[3]);

/* ---- the active-set update on a partitioned mesh (hanging nodes included): pfm_active_set_device in pieces that a rank
 * with ghost peers can compose, and the composition in one collective call.  The solution, the residual and the flag
 * bytes stay on the device; per Newton step one byte per halo node travels next to the halo values. */

/* The active-set predicate of cracks.cc:2837-2886 and the cycle counter of 2903-2909 WITHOUT the re-distribution of
 * 2888-2890: the arguments, criterion, rounding (no fused multiply-add), cycle counter, phi := phi_old, flag bit `dim`
 * and counts of pfm_active_set_device (the same kernel), over the owned nodes that do not hang, on ANY context -- a
 * partitioned one with hanging nodes too.  Hanging nodes keep their (now stale) values in d_solution until
 * pfm_distribute_hanging_device; ghost flag bytes are not touched (pfm_halo_exchange_flags).  Synchronous. */
int pfm_active_set_owned_device(pfm_ctx *ctx, const double *d_residual_total, const double *d_mass, double c,
                                double *d_solution, const double *d_old_solution, int32_t *d_cycle_counter,
                                int64_t counts[3]);

/* The import of the ghost nodes' active-set lines (what IndexSet active_set_locally_relevant / constraints_update hold of
 * other ranks' dofs after cracks.cc:2826-2890).  The message is ONE BYTE per node, the flag byte of the context; the
 * message of peer k starts at byte send_ptr[k] resp. recv_ptr[k] of the lists given to pfm_halo_register.
 * PFM_HALO_DOUBLES_PER_NODE and the messages of pfm_halo_pack_all / pfm_halo_exchange are not affected.
 *   pack:    d_buf_all[j] = flag byte of send node j                              (device buffer, n_send bytes)
 *   unpack:  bit `dim` (the active-set line of the phase field) of d_buf_all[j] replaces bit `dim` of the flag byte of
 *            ghost node recv_nodes[j]; its displacement bits stay what pfm_set_constraints gave -- they are
 *            set_newton_bc's (cracks.cc:2711-2714) and do not change inside the Newton loop.  Owned nodes are never
 *            written.
 * Asynchronous on the context's stream.  A context without peers: PFM_OK, nothing launched. */
int pfm_halo_pack_flags_all(pfm_ctx *ctx, uint8_t *d_buf_all);
int pfm_halo_unpack_flags_all(pfm_ctx *ctx, const uint8_t *d_buf_all);
/* pack -> one grouped ncclSend / ncclRecv per peer (ncclUint8) on the context's stream -> unpack, in message buffers of
 * the context (allocated at the first call, counted in pfm_ctx_device_bytes).  The handle rules, the error path (a failure
 * after the group has been opened aborts an owned communicator and disables the handle) and the collective rule (every
 * rank of a peer pair calls it, in the same order relative to its other exchanges) are pfm_halo_exchange's.  Like that
 * entry it is launch-ready but has NOT run between two ranks yet; the protocol is tested with in-process copies of the
 * pack / unpack buffers.  A context without peers: PFM_OK, nothing launched, comm may be NULL. */
int pfm_halo_exchange_flags(pfm_ctx *ctx, void *comm, const int *peer_ranks);

/* constraints_hanging_nodes.distribute(solution) (cracks.cc:2888-2890 after the active set, and 2788 after
 * set_initial_bc) for a context whose hanging nodes may have ghost parents.  For every local hanging node, owned or ghost,
 * and every component:  value = sum_j hn_weights[j] * parent_j  in table order, where the parents are read from the
 * context's node arrays of the solution (as last scattered by pfm_state_set / pfm_state_set_solution and imported by the
 * halo) and the result is written to those arrays; for OWNED hanging nodes it is also written to d_solution (device vector
 * over the owned dofs in the context's layout; may be NULL: node arrays only).  phi_old / phi_oldold are not touched.
 * Ghost hanging nodes are recomputed here and not imported: their parents are local nodes (the ghost layer is closed under
 * the hanging table), so no second exchange follows.  The table is closed (parents never hang): the reads and the writes
 * are disjoint and the call is idempotent.  On an unpartitioned context the values equal what pfm_active_set_device leaves
 * in d_solution bit for bit (one device function forms the sum in both).  Asynchronous on the context's stream.  A context
 * without hanging nodes: PFM_OK, nothing launched. */
int pfm_distribute_hanging_device(pfm_ctx *ctx, double *d_solution /* may be NULL */);

/* cracks.cc:2826-2890 on a rank with ghost peers, in one collective call:
 *   pfm_active_set_owned_device(...);  pfm_state_set_solution(d_solution, on_device = 1);
 *   the halo values (pfm_halo_exchange's messages) and the flag bytes (pfm_halo_exchange_flags' messages) in ONE RCCL group;
 *   pfm_distribute_hanging_device(d_solution).
 * Afterwards d_solution, the context's node state (solution fields; phi_old / phi_oldold are re-imported with their
 * unchanged values) and its flag bytes are what the next pfm_assemble_device needs, ghosts included.  counts are THIS
 * rank's: the caller sums them (Utilities::MPI::sum, cracks.cc:2893-2895, 2914).  comm, peer_ranks: as pfm_halo_exchange;
 * on a context without peers comm may be NULL, nothing is exchanged and d_solution, the flags, the cycle counters and the
 * counts equal pfm_active_set_device's bit for bit (which does not scatter the node state; this call does).
 * With peers it is launch-ready but has NOT run between two ranks yet (see pfm_halo_exchange_flags).
 * PFM_ERR_BAD_ARG with nothing launched: a NULL context, vector or counts; peers without comm or peer_ranks. */
int pfm_active_set_exchange(pfm_ctx *ctx, void *comm, const int *peer_ranks, const double *d_residual_total,
                            const double *d_mass, double c, double *d_solution, const double *d_old_solution,
                            int32_t *d_cycle_counter, int64_t counts[3]);

/* What the line search reads after every assemble_nl_residual() (cracks.cc:2946-2949; 10-50 times per Newton step) and the
 * Newton loop after every assembly (cracks.cc:2791-2794, 2918-2919): the norms of a residual vector with the constrained
 * lines zeroed -- constraints_update.set_zero(system_pde_residual); system_pde_residual.l2_norm() -- without the vector
 * ever leaving the device (24 bytes instead of 2 x 327 MB at 216^3).
 *   d_residual: device vector over the owned dofs in the context's layout (residual_pde of pfm_assemble_device /
 *   pfm_assemble_nl_residual_device, or residual_total); zeroed lines = the flag bits last given to pfm_set_constraints
 *   (Dirichlet lines, active set) and every component of a hanging node.
 *   out[0] = l2 norm, out[1] = l-infinity norm, out[2] = sum of squares -- of THIS rank's owned dofs; a partitioned caller
 *   adds out[2] over the ranks and takes the root (Utilities::MPI::sum inside l2_norm), and the maximum of out[1].
 * Deterministic two-stage reduction (the grid depends on n_owned only); ordered behind the assembly on the context's
 * stream; synchronous, out is a host pointer. */
int pfm_residual_norms(pfm_ctx *ctx, const double *d_residual, double out[3]);

/* read back the flag byte of every local node (bit c: dof (node,c) has a homogeneous constraint line) */
int pfm_get_constraints(pfm_ctx *ctx, uint8_t *node_flags);

/* compute_energy + compute_tcv on the node state last given to pfm_state_set (after the ghost import):
 *   out[0] = bulk energy   int ((1+k) pf^2 + k) psi(E)                          cracks.cc:3677
 *   out[1] = crack energy  G_c/2 int ((pf-1)^2/eps + eps |grad pf|^2)            cracks.cc:3679-3680
 *   out[2] = TCV           int u . grad pf                                       cracks.cc:3587
 * over the cells with cell_owned[cell] != 0 (host array [n_cells]; NULL = every local cell), this rank's
 * part of the sums (the caller adds the ranks, Utilities::MPI::sum, cracks.cc:3590, 3685-3686).
 * Deterministic two-stage reduction; synchronous, out is a host pointer. */
int pfm_functionals(pfm_ctx *ctx, const uint8_t *cell_owned, double out[3]);
/* The same with the Lame coefficients of the energy given per cell (host arrays [n_cells]; both NULL = the context's,
 * i.e. pfm_functionals).  Needed for the reference's heterogeneous test case: assemble_system adds 1.0 to the
 * Young's modulus read from the bitmap (cracks.cc:2209-2210) but compute_energy does not (cracks.cc:3649-3657), so
 * the energy is NOT evaluated with the coefficients the assembly uses; a caller that wants the reference's
 * statistics passes the un-shifted ones here. */
int pfm_functionals_material(pfm_ctx *ctx, const uint8_t *cell_owned, const double *cell_lambda, const double *cell_mu,
                             double out[3]);

/* The remaining functionals of the reference's statistics (pfm_postproc.hip).  Same contract as pfm_functionals: they
 * read the node state last given to pfm_state_set / pfm_state_set_solution (after the ghost import), return THIS RANK's
 * part (the caller does Utilities::MPI::sum and the scaling the reference applies after it), are ordered behind earlier
 * work on the context's stream and synchronous with host outputs.  Deterministic fixed-order reductions: repeated calls
 * are bitwise identical.  PFM_ERR_BAD_ARG, with nothing launched, before pfm_set_params and on bad input (a cell out of
 * range, a face >= 2 dim, lines not finite and strictly ascending, a negative count or eps, a NULL output). */

/* compute_load (cracks.cc:3726-3790): out[d] = sum over the given (cell, face) pairs of
 *   int_face (lambda tr(E) I + 2 mu E) n dA,   E = sym grad u,  QGauss<dim-1>(3),  MappingQ1,  outward normal,
 * with lambda, mu = the GLOBAL coefficients of pfm_set_params even when per-cell ones are set (as the reference,
 * cracks.cc:3776-3777).  Faces in deal.II numbering: 2 d = lower, 2 d + 1 = upper face of reference axis d.  out has dim
 * entries, the raw vector: the sign flips of cracks.cc:3793-3815 are the caller's.  A deal.II host passes the faces of its
 * owned cells with cell->face(f)->at_boundary() && boundary_id() == 3. */
int pfm_face_load(pfm_ctx *ctx, int64_t n_faces, const int32_t *cells, const uint8_t *faces, double *out);

/* compute_cod(lines[i]) for all lines at once (cracks.cc:3453-3550) over the cells with cell_owned[cell] != 0 (NULL =
 * every local cell): a face of such a cell matches line x when
 *   not (center_x - diameter > x), not (center_x + diameter < x), |n(q0) . e_x| >= 0.5, x - eps < q0_x < x + eps
 * (q0 = face quadrature point 0), and
 *   cod[i]     = sum over the faces matching lines[i] of int_face 0.5 u . grad(phi) dA   (BEFORE the /2 and the MPI sum of
 *                cracks.cc:3538-3539: interior faces are counted from both cells, as in the reference)
 *   n_faces[i] = number of those faces (the caller returns -1e300 when the global count is 0).
 * A face may match several lines.  lines: strictly ascending (the reference's x_i = -1.5 + i / 256, cracks.cc:3716-3720,
 * with eps = 1e-8).  The (line, cell, face) list of the first call is cached in the context for the same lines, eps and
 * mask: later calls only evaluate the faces. */
int pfm_cod_lines(pfm_ctx *ctx, const uint8_t *cell_owned, int n_lines, const double *lines, double eps, double *cod,
                  int64_t *n_faces);

/* compute_cod_array (cracks.cc:3337-3449; the reference has its call switched off at cracks.cc:4491, "very expensive"): the
 * Sneddon COD profile, the integral of u . grad(phi) binned into n_buckets slices along x with QIterated(QMidpoint, n_sub).
 * Every cell with cell_owned[cell] != 0 (NULL = every local cell) is sampled at the n_sub^dim points xi_d = (k_d + 0.5) / n_sub
 * (k_0 fastest), weight n_sub^-dim each; at each point, with MappingQ1, x = x(xi)[0], JxW = det J(xi) * weight and
 *   idx = floor((x - x_lo) / (x_hi - x_lo) * n_buckets + 0.5)      (value_to_bucket, cracks.cc:3323-3328, with its constants
 *                                                                   made arguments; in double, in this order, unfused)
 * points with idx < 0 or idx >= n_buckets are dropped (cracks.cc:3393-3394), otherwise
 *   values[idx] += (u . grad phi) JxW,   volume[idx] += JxW         (cracks.cc:3404-3409).
 * values, volume: host out [n_buckets], THIS rank's raw sums; the MPI sum, the "/ width / 2.0" of cracks.cc:3419 and the
 * error norm of 3432-3438 are the caller's.  The reference's call is (75, -1.5, 1.5, 100).
 * Limits: 1 <= n_buckets <= 128, 1 <= n_sub <= 128, x_lo < x_hi and both finite, non-NULL outputs; anything else is
 * PFM_ERR_BAD_ARG with nothing launched and the outputs untouched.
 * No floating-point atomics: a wave walks the rows of a fixed slab of a cell's points (256 rows along xi_0), a fixed number of
 * waves takes the (cell, slab) items in contiguous ranges, and the per-wave partial sums are added in wave order; the order of
 * every sum depends on the mesh size and the arguments only, so repeated calls are bitwise identical.  One launch covers at
 * most 2^32 sample points (the bound and what is known about its kernel time: DESIGN.md 4.4): the host side splits the cell range, launch after
 * launch on the context's stream, and the launches' sums are added in launch order.  The scratch (at most 12 MiB + 4 KiB) is kept in the
 * context and counted in pfm_ctx_device_bytes. */
int pfm_cod_buckets(pfm_ctx *ctx, const uint8_t *cell_owned, int n_buckets, double x_lo, double x_hi, int n_sub,
                    double *values /* host out [n_buckets] */, double *volume /* host out [n_buckets] */);

/* The point evaluation behind compute_point_stress (cracks.cc:3285-3320: GridTools::find_active_cell_around_point, then
 * values / gradients of the solution at the point) and compute_point_value (cracks.cc:3264-3283).
 *   points  host [n_points][dim]
 *   cell    host out [n_points]: the cell the point was evaluated in, or -1
 *   values  host out [n_points][dim+1] or NULL: the Q1 interpolant of (u_0 .. u_{dim-1}, phi)
 *   grads   host out [n_points][dim+1][dim] or NULL: grads[p][c][d] = d(component c) / d x_d
 * Cell rule (a DEVIATION from deal.II, which walks the cells around the vertex closest to the point): cell[p] is the
 * LOWEST-numbered cell with cell_owned[cell] != 0 (NULL = every local cell) for which the Newton inverse of the Q1 map
 * converges to a xi with every coordinate in [-1e-10, 1 + 1e-10] (find_active_cell_around_point's default tolerance).  The
 * inverse is attempted only for cells whose vertex bounding box, inflated by 1e-8 * the cell diameter, contains the point;
 * it starts at the cell centre, takes at most 20 steps and has converged when a step is at most 1e-12 in every coordinate; an
 * inverse that does not converge is no candidate.  Inside a cell both rules pick that cell; on a face or a vertex the
 * gradient is discontinuous and the reference's choice depends on the rank, this one on the cell numbers only.
 * Evaluation: xi is clamped to the unit cell (project_to_unit_cell, cracks.cc:3306).  The entries of a point without a cell
 * are written as 0.0.  On a partitioned context the caller passes its owned-cell mask and takes the values of the rank
 * whose cell >= 0 (Utilities::MPI::max in the reference).
 * PFM_ERR_BAD_ARG with nothing launched and the outputs untouched: n_points outside 0 .. 4096, a non-finite coordinate, a
 * NULL points or cell.  Integer atomics only: deterministic. */
int pfm_point_eval(pfm_ctx *ctx, const uint8_t *cell_owned, int n_points, const double *points /* host [n_points][dim] */,
                   int32_t *cell /* host out [n_points] */, double *values /* host out [n_points][dim+1] or NULL */,
                   double *grads /* host out [n_points][dim+1][dim] or NULL */);

/* VectorTools::integrate_difference(..., ExactPhiSneddon(alpha_eps), QGauss<dim>(3), L2_norm, phi only) (cracks.cc:4495-4516,
 * 418-450; exact phi = 1 - exp(-dist / alpha_eps), dist = distance to the segment [-1, 1] x {0}, alpha_eps of pfm_set_params):
 * *sum_sq = sum over the cells with cell_owned[cell] != 0 (NULL = all) of int_cell (phi_h - phi_exact)^2 dx, in double.
 * The caller takes the root of the MPI sum.  The reference keeps every cell's error in a Vector<float>: its printed
 * phi_L2_error carries a float rounding (about 1e-7 relative) that this sum does not. */
int pfm_sneddon_phi_error(pfm_ctx *ctx, const uint8_t *cell_owned, double *sum_sq);

/* ---- mesh adaptation (pfm_adapt.hip): the two sweeps around the context rebuild of refine_mesh() (cracks.cc:3895-4163)
 * and the other half of determine_mesh_dependent_parameters() (cracks.cc:3820-3836).  Conventions of the functionals above:
 * PFM_ERR_BAD_ARG with nothing launched on bad input, ordered behind earlier work on the context's stream, synchronous
 * where outputs are host pointers, deterministic (repeated calls are bitwise identical). */

typedef struct
{
  double phi_threshold; /* flag a cell when phi < threshold at one of its vertices (strict <; NaN never flags),
                           cracks.cc:3987-3992, 4026-4031, 4060-4065; NaN = criterion off */
  int use_box;          /* also flag a cell with a vertex in the closed box [box_lo, box_hi] (first `dim` entries; +-inf for
                           open sides): fixed_preref_* 3911-3921, 3934-3944, 3957-3967 and the y >= 1.75 rule of 4007-4017 */
  double box_lo[3], box_hi[3];
  int max_level;        /* flags of cells with cell_level[cell] == max_level are cleared afterwards (4107-4116);
                           < 0: no limit (Sneddon) */
} pfm_refine_criteria;

/* The refinement indicator of refine_mesh() on the node state last given to pfm_state_set / pfm_state_set_solution (after
 * the ghost import; the contract of pfm_functionals: an owned cell may have ghost vertices), on every kernel path.
 *   cell_owned  host [n_cells] or NULL = every local cell; cells that are not owned are never flagged
 *   cell_level  host [n_cells]; may be NULL iff max_level < 0
 *   flags       host out [n_cells], 0 / 1 -- what the host passes to cell->set_refine_flag()
 *   n_flagged   host out, flagged cells of THIS rank (the caller does the MPI sum of cracks.cc:4133)
 * One byte per cell and eight bytes travel to the host, not the solution. */
int pfm_refine_flags(pfm_ctx *ctx, const pfm_refine_criteria *crit, const uint8_t *cell_owned, const uint8_t *cell_level,
                     uint8_t *flags, int64_t *n_flagged);

/* min over the cells with cell_owned[cell] != 0 (NULL = all) of cell->diameter(), the largest vertex distance of the
 * cell (cracks.cc:3824-3835) -- what the h-dependent kappa and eps need after every rebuild.  +inf where no cell is
 * masked; the caller takes the minimum over the ranks. */
int pfm_min_cell_diameter(pfm_ctx *ctx, const uint8_t *cell_owned, double *h_min);

/* SolutionTransfer::interpolate for refinement (cracks.cc:4137-4159) between two contexts: n_vectors dof vectors of `src`
 * (device, src's layout) are interpolated to dof vectors of `dst` (device, dst's layout).
 *   parent_cell[c]  the cell of src that dst cell c is identical to (child[c] == 255) or an isotropic child of
 *   child[c]        255, or the child number 0 .. 2^dim - 1 in deal.II order: bit d = offset along reference axis d
 * (host arrays [dst n_cells]).  The value at vertex v of dst cell c is the parent's Q1 function at the reference point
 * xi_d = (child bit d + vertex bit d) / 2: the weights 1, 1/2, 1/4, 1/8 are exact, the terms with a non-zero weight are
 * added in ascending parent-vertex order, and every dst node takes its value from the lowest-numbered dst cell that has
 * it.  src vectors are expected distributed at hanging nodes (as cracks.cc:4417 leaves them).
 * Before anything is written the relation is checked on the device against the coordinates: every dst vertex must lie at
 * the Q1 image of its xi within 1e-10 of the parent's diameter.  A mismatch, an index out of range or a bad child number
 * is PFM_ERR_BAD_ARG and d_dst is untouched.
 * Both contexts must be unpartitioned (n_owned_nodes == n_nodes), on the same device, of the same dimension and layout,
 * 1 <= n_vectors <= 8: anything else is PFM_ERR_UNSUPPORTED (p4est repartitions at a refinement; that transfer stays the
 * host's).  Coarsening is NOT supported: the reference's phase-field strategies never set a coarsen flag.
 * Ordered behind earlier work on both contexts' streams; the values are written on dst's stream (asynchronous after the
 * check).  src must stay alive until the call has returned. */
int pfm_state_transfer(pfm_ctx *src, pfm_ctx *dst, const int32_t *parent_cell, const uint8_t *child, int n_vectors,
                       const double *const *d_src, double *const *d_dst);

/* ---- RefinementStrategy::mix (cracks.cc:4043-4116): the Kelly indicator of the displacements, zeroed where the phase
 * field has flagged, and refine_and_coarsen_fixed_number(..., top_fraction, 0.0).  All four read the node state last given
 * to pfm_state_set / pfm_state_set_solution (hanging nodes distributed) and work on every kernel path.
 *
 * KellyErrorEstimator<dim>::estimate as the reference calls it (deal.II >= 9: strategy cell_diameter_over_24, empty
 * Neumann map, coefficient 1):
 *   eta[K] = sqrt( h_K / 24 * sum over the faces F of K of I_F ),   h_K = cell->diameter() as in pfm_min_cell_diameter,
 *   I_F    = int_F sum_{c in mask} ( n . grad u_c |_K - n . grad u_c |_K' )^2 dA,   QGauss<dim-1>(3), MappingQ1 on both sides.
 * A face whose neighbour is refined once more contributes the sum of its 2^(dim-1) subface integrals (each evaluated from
 * the fine cell's side, added in ascending fine-cell order), a fine cell's face against a coarser neighbour that one
 * subface; a face without a neighbour among the local cells -- domain boundary, slit lips with duplicated nodes, a cell of
 * another rank that is not in the ghost layer -- contributes 0.
 *   cell_owned      host [n_cells] or NULL = every local cell; eta = 0 for the others
 *   component_mask  bit c < dim: displacement component c, bit dim: phi.  The reference uses (1 << dim) - 1.  0 or a bit
 *                   above dim: PFM_ERR_BAD_ARG
 *   d_eta           device out [n_cells], double.  Asynchronous on the context's stream, like pfm_diag_mass_device.
 * The indicator is computed and returned in double; the reference accumulates into a Vector<float>, so its values (and a
 * threshold derived from them) carry a float rounding that these do not (see pfm_sneddon_phi_error).
 * The face-neighbour table is built from the cell and hanging-node tables of pfm_ctx_create at the first call, kept in
 * the context and counted in pfm_ctx_device_bytes (PFM_ERR_NOMEM if it does not fit; the context stays usable).  A face
 * matches the cell with the same vertex set; an unmatched face with a hanging vertex matches the face made of its other
 * vertices and the parents (as listed in hn_parents) of the hanging ones.
 * Partitioned contexts: the caller's contract is that every face neighbour of an owned cell is a local cell (p4est's
 * ghost layer holds them) and that the ghost values have been imported; eta is then right for every owned cell.
 * No floating-point atomics: repeated calls are bitwise identical. */
int pfm_kelly_indicator(pfm_ctx *ctx, const uint8_t *cell_owned, unsigned component_mask, double *d_eta);

/* The k-th largest value (1-based) of the device array d_ind [n_cells] over the cells with cell_owned[cell] != 0 (NULL =
 * all): exact (radix select on the order-preserving 64-bit key with integer histograms).  -0.0 and 0.0 compare equal (0.0
 * is returned), a NaN ranks below every number (a NaN is returned when rank k falls on one).
 *   counts[0] = masked values above *threshold, counts[1] = masked values equal to it.
 * k < 1 or k above the number of masked cells: PFM_ERR_BAD_ARG.  Synchronous. */
int pfm_indicator_select(pfm_ctx *ctx, const double *d_ind, const uint8_t *cell_owned, int64_t k, double *threshold,
                         int64_t counts[2]);

/* The same two counts for a given t.  A distributed host bisects on this with its own MPI sum, as
 * parallel::distributed::GridRefinement does; the library does not do the bisection.  Synchronous. */
int pfm_indicator_count(pfm_ctx *ctx, const double *d_ind, const uint8_t *cell_owned, double t, int64_t counts[2]);

/* cracks.cc:4043-4116 on one rank:
 *   (a) the flags of `crit` without its level limit (pfm_refine_flags),
 *   (b) eta = pfm_kelly_indicator(component_mask), set to 0 on the flagged cells (4085-4095),
 *   (c) k = (int64) (top_fraction * n_cells), truncated as the reference's static_cast.  k >= 1: t = the k-th largest eta
 *       over all local cells; t == 0 becomes the smallest positive eta; every cell with eta >= t is flagged -- ties at t
 *       all flag, a zero indicator never does (serial refine_and_coarsen_fixed_number + refine),
 *   (d) flags at crit->max_level are cleared (4107-4116).
 * Outputs as pfm_refine_flags, plus *threshold = the t used (+inf when (c) flags nothing: k == 0 or no positive eta).
 * top_fraction outside [0, 1] or a bad mask: PFM_ERR_BAD_ARG.  A partitioned context (n_owned_nodes != n_nodes) is
 * PFM_ERR_UNSUPPORTED with the outputs untouched: the fraction is of the global cell count, so that host composes the three
 * calls above itself.  Synchronous. */
int pfm_refine_flags_mix(pfm_ctx *ctx, const pfm_refine_criteria *crit, double top_fraction, unsigned component_mask,
                         const uint8_t *cell_owned, const uint8_t *cell_level, uint8_t *flags, int64_t *n_flagged,
                         double *threshold);

/* ---- the Newton line search (pfm_linesearch.hip): cracks.cc:2942-2957 (active-set Newton) and 3048-3062 (plain Newton),
 *   for (step = 0; step < max_steps; ++step)
 *     { solution += newton_update;  assemble_nl_residual();  set_zero;  norm;  if (norm < newton_residual) break;
 *       solution = saved_solution  |  solution -= newton_update;   newton_update *= line_search_damping; }
 * with the vectors on the device.  All vectors are device dof vectors over the owned dofs in the context's layout.
 *
 * Rounding is part of the contract: every +, - and * below is ONE IEEE double operation rounded on its own, never a fused
 * multiply-add, so that the results equal an unfused host statement (numpy, the reference's vector classes) bit for bit and
 * a host can reproduce `solution` from the step count alone.  In SUBTRACT mode fl(fl(s + u) - u) is in general not s: that
 * drift is the reference's behaviour (cracks.cc:3059) and is kept. */
enum { PFM_LS_NORM_L2 = 0, PFM_LS_NORM_LINF = 1 };              /* cracks.cc:2949 / 3054 */
enum { PFM_LS_RESTORE_SAVED = 0, PFM_LS_RESTORE_SUBTRACT = 1 }; /* solution = saved_solution (2955) / solution -= newton_update (3059) */

typedef struct pfm_line_search_opts {
  int32_t max_steps;   /* >= 1 */
  int32_t norm;        /* PFM_LS_NORM_* */
  int32_t restore;     /* PFM_LS_RESTORE_* */
  int32_t reserved;    /* 0 */
  double  damping;     /* finite */
  double  reference;   /* newton_residual the trial must beat: accepted iff trial < reference (strict; NaN never accepts) */
} pfm_line_search_opts;

typedef struct pfm_line_search_result {
  int32_t steps;        /* the reference's line_search_step at loop exit: 0 .. max_steps */
  int32_t accepted;     /* 1 iff the loop left through the break */
  double  norms[3];     /* pfm_residual_norms of the LAST trial's residual_pde: l2, linf, sum of squares */
  double  linf_block[2];/* linf of its displacement dofs / phase-field dofs, lines zeroed (cracks.cc:3070-3071) */
} pfm_line_search_result;

/* The vector statements, one pass over the vectors each, for any context (a partitioned one too: owned dofs only),
 * asynchronous on the context's stream.
 *   advance:            saved = solution (d_saved != NULL);  solution = solution + update
 *   retreat, SAVED:     solution = saved;              update = update * damping;  advance != 0: solution = saved + update
 *   retreat, SUBTRACT:  solution = solution - update;  update = update * damping;  advance != 0: solution = solution + update
 * (the update of the `advance` half is the damped one: the fused pass is the tail of one rejected trial and the head of the
 * next).  PFM_ERR_BAD_ARG with nothing launched: a NULL solution or update, an unknown restore mode, a non-finite damping,
 * SAVED mode without d_saved. */
int pfm_line_search_advance(pfm_ctx *ctx, double *d_solution, const double *d_update, double *d_saved /* NULL or out */);
int pfm_line_search_retreat(pfm_ctx *ctx, int restore, double damping, double *d_solution, double *d_update,
                            const double *d_saved /* SAVED mode */, int advance);

/* The whole loop in one call: trial 0 is `advance`, trial k > 0 the fused `retreat(advance = 1)`; every trial then runs
 * pfm_assemble_nl_residual_device(d_solution, d_residual_pde, d_residual_total) as it is and the norm stage, and the
 * compare is made on the host (one synchronisation per trial); a rejected last trial is followed by `retreat(advance = 0)`.
 *   out->norms are bitwise what pfm_residual_norms returns for d_residual_pde (same grid, same reduction order), and
 *   max(out->linf_block) == out->norms[1] exactly.  The trial value is norms[0] (L2) or norms[1] (LINF); a NaN trial is
 *   never accepted.
 * On exhaustion (steps == max_steps, accepted == 0) d_solution is restored per mode and d_update has been damped max_steps
 * times, but d_residual_pde, d_residual_total, norms and linf_block are those of the LAST TRIAL, not of the restored
 * solution -- what the reference leaves behind (residual_relevant, new_newton_residual of cracks.cc:2947-2949).
 * The context's node state is whatever the last pfm_assemble_nl_residual_device left, i.e. the last trial's solution, also
 * after an exhausted search: a caller that next uses an entry reading the node state (functionals, refinement flags, a
 * Jacobian through pfm_assemble_device) calls pfm_state_set_solution(d_solution) first, as it must after that entry today.
 * The saved_solution of SAVED mode is a buffer of the context, allocated at the first use and counted in
 * pfm_ctx_device_bytes; PFM_ERR_NOMEM with nothing touched if it cannot be allocated.
 * Contexts without halo peers only (PFM_ERR_BAD_ARG with peers, like pfm_assemble_nl_residual_device: such a rank composes
 * the loop from the two statements above, its ghost import, the assembly and pfm_residual_norms).
 * PFM_ERR_BAD_ARG with nothing launched and nothing written: max_steps < 1, an unknown norm or restore, a non-finite
 * damping, a NULL pointer. */
int pfm_line_search_device(pfm_ctx *ctx, const pfm_line_search_opts *opts, double *d_solution, double *d_update,
                           double *d_residual_pde, double *d_residual_total, pfm_line_search_result *out);

/* project_back_phase_field (cracks.cc:3111-3137) on the owned phase-field dofs of a device vector in the context's layout:
 * x := std::max(0.0, std::min(x, 1.0)), i.e. NaN -> +0.0, -0.0 -> +0.0, -inf -> +0.0, +inf -> 1.0; displacement dofs are
 * untouched.  Any context; asynchronous on the context's stream. */
int pfm_project_back_device(pfm_ctx *ctx, double *d_solution);

#ifdef __cplusplus
}
#endif
#endif

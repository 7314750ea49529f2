/* pfm_assemble.h — C ABI of the MI355X-native Newton residual/Jacobian assembly.
 *
 * Drop-in boundary for ONE path of tjhei/cracks:
 *   FracturePhaseFieldProblem<dim>::assemble_system(bool residual_only)   cracks.cc:2129-2498
 *   FracturePhaseFieldProblem<dim>::assemble_nl_residual()                cracks.cc:2507-2512
 * The reference has no plugin/FFI interface for it (assemble_system is a private member,
 * cracks.cc:1039-1040); this header defines the interface a deal.II glue shim binds
 * (INTEGRATION.md).  Semantics = cracks.cc:2133-2475 minus deal.II object handling:
 * zero the outputs, import ghost values, integrate every cell, scatter through the
 * constraints, reduce.  The AMG set-up at cracks.cc:2477-2497 stays with the caller.
 *
 * Plain C, POD only.  Every entry point returns a pfm_status (0 = ok) and never
 * aborts/exits/throws (the reference's abort() at cracks.cc:1735 becomes
 * PFM_ERR_NOT_ORTHOGONAL).  A context is not re-entrant; different contexts are
 * independent.  One context <-> one GPU <-> one reference MPI rank (cracks.cc:4587).
 *
 * Index spaces.  Nodes are numbered per rank: owned nodes [0,n_owned) first, ghost
 * nodes [n_owned,n_nodes) after (the "locally relevant" numbering of cracks.cc:1622-1628).
 * Local dof i of a cell <-> (vertex i/(dim+1), component i%(dim+1)); components
 * 0..dim-1 = displacement, dim = phase field (cracks.cc:980-996).
 *
 * Dof vectors (solution / residual) hold OWNED dofs only, in one of the reference's two
 * numberings (cracks.cc:1587-1590):
 *   PFM_LAYOUT_INTERLEAVED  one block,  dof = node*(dim+1)+comp      (direct solver)
 *   PFM_LAYOUT_BLOCKED      [u | phi],  u dof = node*dim+comp, phi dof = n_owned*dim+node
 * Matrix values are CSR, rows = owned dofs, columns in the rank-local numbering (ghost columns
 * included), ascending within a row unless pfm_pattern_bind() adopted another order from the host;
 * full component coupling (cracks.cc:1644-1654):
 *   INTERLEAVED: block 0 only;   BLOCKED: 0 = (u,u), 1 = (u,phi), 2 = (phi,u), 3 = (phi,phi)
 * The pattern is the node graph of the constraint-resolved mesh tensor the component
 * coupling; pfm_pattern_get() returns it, pfm_pattern_bind() adopts the host's own arrays.
 */
#ifndef PFM_ASSEMBLE_H
#define PFM_ASSEMBLE_H

#include <stdint.h>
#include "pfm_params.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pfm_status
{
  PFM_OK = 0,
  PFM_ERR_BAD_ARG = 1,
  PFM_ERR_HIP = 2,            /* a HIP runtime call failed; pfm_last_error() has the text */
  PFM_ERR_NOT_ORTHOGONAL = 3, /* eigenvector sanity check failed (reference abort(), cracks.cc:1732-1736) */
  PFM_ERR_NONFINITE = 4,      /* non-finite value in an output (checked by pfm_check_finite only) */
  PFM_ERR_UNSUPPORTED = 5,    /* e.g. stress split in 3-D (reference is 2-D only, cracks.cc:1685-1690) */
  PFM_ERR_NOMEM = 6,
  PFM_ERR_COMM = 7,           /* an RCCL call failed; pfm_last_error() has the text */
  PFM_ERR_INTERNAL = 8        /* an invariant of the library was violated (e.g. the deferred-patch list overflowed) */
} pfm_status;

enum
{
  PFM_LAYOUT_INTERLEAVED = 0,
  PFM_LAYOUT_BLOCKED = 1
};

/* per-dof constraint flag bits, one byte per NODE, bit c = component c */
enum
{
  PFM_NODE_ALLCOMP_MASK = 0x0f
};

typedef struct pfm_ctx pfm_ctx;

/* Static description of the rank-local mesh; everything is copied. Replaces the
 * DoFHandler / FEValues / Triangulation inputs of cracks.cc:2156-2203. */
typedef struct pfm_mesh_desc
{
  int32_t dim;               /* 2 or 3 */
  int32_t layout;            /* PFM_LAYOUT_* */
  int32_t n_nodes;           /* owned + ghost */
  int32_t n_owned_nodes;
  int64_t n_cells;           /* all local cells whose contributions reach an owned row:
                                owned cells + one ghost layer ("owner computes") */
  const int32_t *cell_nodes; /* [n_cells][2^dim], deal.II vertex order */
  const double *coords;      /* [n_nodes][dim] */
  const double *cell_lambda; /* [n_cells] or NULL: per-cell Lame override (cracks.cc:2207-2216) */
  const double *cell_mu;
  /* closed hanging-node table (constraints_hanging_nodes, cracks.cc:1630-1635), node level:
   * node hn_nodes[k] = sum_j hn_weights[j]*parent hn_parents[j], j in [hn_ptr[k],hn_ptr[k+1]) */
  int32_t n_hanging;
  const int32_t *hn_nodes;
  const int64_t *hn_ptr;
  const int32_t *hn_parents;
  const double *hn_weights;
  /* structured fast path hint: cells form an nx*ny(*nz) box in lexicographic order with
   * lexicographic node numbering (all zero = unknown; the library verifies the claim). */
  int32_t box_cells[3];
} pfm_mesh_desc;

/* -- life cycle ---------------------------------------------------------------------- */
/* Build a context on HIP device `device`.  Must be rebuilt after every setup_system()
 * (cracks.cc:4148, 4174). */
int pfm_ctx_create(pfm_ctx **out, const pfm_mesh_desc *mesh, int device);
int pfm_ctx_destroy(pfm_ctx *ctx);
const char *pfm_last_error(const pfm_ctx *ctx);
/* all launches/copies go to this hipStream_t (default: the null stream) */
int pfm_ctx_set_stream(pfm_ctx *ctx, void *hip_stream);

/* -- inputs set elsewhere but consumed by assemble_system -------- */
int pfm_set_params(pfm_ctx *ctx, const pfm_params *prm);
/* Which law a stress-split assembly (decompose_stress_matrix > 0 && timestep_number > 0, cracks.cc:2294) uses.
 *   PFM_SPLIT_REFERENCE  the reference's closed form (decompose_stress, cracks.cc:1923-2120): 2-D only -- compiled for
 *                        dim = 3 it reads the 2 x 2 corner of the strain (cracks.cc:1683-1690) -- so pfm_set_params refuses
 *                        a split assembly of a 3-D context with PFM_ERR_UNSUPPORTED.  Default.
 *   PFM_SPLIT_SPECTRAL   3-D contexts: the Miehe-type split through the three eigenpairs of the strain (DESIGN.md §2,
 *                        cracks_amd/split3d.py); never PFM_ERR_NOT_ORTHOGONAL.  A 3-D box or overlay context runs a split
 *                        assembly through the general family over all cells and returns to its own kernels with the split
 *                        off (timestep_number = 0).
 *   PFM_SPLIT_VOLDEV     3-D contexts: the volumetric-deviatoric split of Amor, Marigo and Maurini (DESIGN.md §2,
 *                        cracks_amd/split3d.py: voldev_split): sigma+ = K max(tr E, 0) I + 2 mu dev E, sigma- = K min(tr E, 0) I,
 *                        K = lambda + 2 mu / 3.  No eigen-solve, an isotropic tangent per q-point; never
 *                        PFM_ERR_NOT_ORTHOGONAL.  Routed like model 1.  Unlike model 1, the cells at hanging vertices keep
 *                        the scratch + ordered gather by default, so a model-3 assembly is bitwise reproducible run to run
 *                        (PFM_HANGING_ATOMIC=1: the atomic class; model 1 is under PFM_HANGING_MODE_GATHER, see
 *                        pfm_set_hanging_mode).  The tangent is discontinuous at tr E = 0 (h(0) = 1, zero
 *                        counts as tension) and follows the sign of the trace the device computes: where tr E is zero up to
 *                        rounding (a pure shear on a general mesh) that sign, and with it the matrix, is not determined.
 * Model 1 or 3 on a 2-D context: PFM_ERR_UNSUPPORTED (2-D keeps the reference's closed form).  An unknown model:
 * PFM_ERR_BAD_ARG -- the value 2 is unassigned and stays refused.  Call it before pfm_set_params; back at model 0 with
 * split parameters still set, a 3-D assembly returns PFM_ERR_UNSUPPORTED.  A living context may change between models 1
 * and 3 at any time: the next assembly uses the new law. */
enum
{
  PFM_SPLIT_REFERENCE = 0,
  PFM_SPLIT_SPECTRAL = 1,
  PFM_SPLIT_VOLDEV = 3
};
int pfm_set_split_model(pfm_ctx *ctx, int model);
/* Which kernels take the residual-only assembly (the line search's call, cracks.cc:2942-2957) of a 3-D context under
 * split law (PFM_SPLIT_VOLDEV, or PFM_SPLIT_SPECTRAL under PFM_SPLIT_ROUTE_LATTICE_ANY) with the split on.
 *   PFM_SPLIT_ROUTE_GENERAL  the general family over all cells, as every split assembly.  Default: nothing about a caller
 *                            that never sets a route changes, bit for bit.
 *   PFM_SPLIT_ROUTE_LATTICE  the row-owner residual kernel of the cartesian family with the law at its q-points
 *                            (k_cart_residual3<false, true>, for every scheme): on a box, on a partitioned sub-box in both
 *                            halves of pfm_assemble_overlapped, and on the level lattices of a 3-D overlay, whose remaining
 *                            cells stay with the general family and its gather.  Full assemblies, model 1, 2-D contexts and a
 *                            context forced to path 0 (pfm_ctx_force_path) run as under PFM_SPLIT_ROUTE_GENERAL.  A Newton step
 *                            then has its Jacobian call's residual_pde from the general family and its line-search
 *                            residuals from the lattice kernels: equal to rounding, not bit for bit.
 *   PFM_SPLIT_ROUTE_LATTICE_ANY  (= 1 | 2) the row-owner residual kernel for every law that has a form there.  Under
 *                            PFM_SPLIT_VOLDEV it is PFM_SPLIT_ROUTE_LATTICE, bit for bit.  Under PFM_SPLIT_SPECTRAL the eigen
 *                            split runs at the q-points of k_cart_residual3<false, false, true> (split_strain<false> and
 *                            split_stress3 of pfm_split3.h, the statements of the general family), on the same lattices and
 *                            halves.  On a 3-D overlay the cells at hanging vertices stay with the general family, which
 *                            by default adds them with atomics under this law: such a residual is equal to the general
 *                            route's to rounding and bitwise reproducible run to run only under PFM_HANGING_MODE_GATHER
 *                            (pfm_set_hanging_mode; a box or a partitioned sub-box always is).  With model 0 it is accepted and has no effect.  The value 2 alone
 *                            is unassigned and stays refused.
 *   PFM_SPLIT_ROUTE_LATTICE_JACOBIAN  (= 1 | 4) PFM_SPLIT_ROUTE_LATTICE, and under PFM_SPLIT_VOLDEV the FULL assembly
 *                            (Jacobian + residual_pde) of a 3-D box or partitioned sub-box on row-owner kernels as well: the
 *                            matrix values by k_cart_split3_jac with the law at its q-points (every value computed by one
 *                            lane and written once, bitwise reproducible and independent of the partition), residual_pde by
 *                            k_cart_residual3<false, true>.  Whole and as both halves of pfm_assemble_overlapped /
 *                            pfm_ctx_force_phase, for every scheme, both layouts, per-cell Lame coefficients and any
 *                            decompose_stress_matrix / decompose_stress_rhs weights.  The residual_pde of the Jacobian call
 *                            and the residual-only (line-search) residuals then come from the same kernel: equal bit for
 *                            bit.  Residual-only calls are those of PFM_SPLIT_ROUTE_LATTICE, bit for bit.  Under model 1 the
 *                            full assembly stays with the general family (the spectral law has no form there) and the route
 *                            acts as PFM_SPLIT_ROUTE_LATTICE (no effect); with model 0 it is accepted and has no effect.  The
 *                            level lattices of a 3-D overlay keep the general family for the full assembly under this route
 *                            (deliberately: their residual-only call follows the route as under 1 and 3), and so does a
 *                            context forced to path 0.  h(tr E) and tr- come from the trace the kernels compute, all three
 *                            from the same statement on the same operands; where tr E of a q-point is zero up to rounding the
 *                            matrix is not determined -- as under the general family, which may then pick the other branch.
 *   PFM_SPLIT_ROUTE_LATTICE_ALL  (= 1 | 2 | 4) the same with the residual-only calls of PFM_SPLIT_ROUTE_LATTICE_ANY: under
 *                            model 1 the residual-only call runs on the lattice kernels, the full assembly does not.
 *                            The values 4 and 6 (the Jacobian bit without bit 1) are refused with PFM_ERR_BAD_ARG.
 *   PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS  (= 1 | 4 | 8) PFM_SPLIT_ROUTE_LATTICE_JACOBIAN, and the level lattices of a 3-D
 *                            overlay (adaptively refined meshes) take the full assembly under PFM_SPLIT_VOLDEV too: every
 *                            regular row (a plain 27-neighbour row of one refinement level) has its matrix values from the
 *                            level form of k_cart_split3_jac and its residual_pde from k_cart_residual3<false, true>; the
 *                            cells that touch another row stay with the general family in its model-3 form, which skips
 *                            the regular rows, with the cells at hanging vertices through scratch and the ordered gather by
 *                            default (PFM_HANGING_ATOMIC=1 and pfm_set_hanging_mode as ever).  The tables, colour lists and
 *                            zeroing are those of an unsplit overlay assembly.  PROMISED: on every regular row residual_pde
 *                            of the full assembly and of the residual-only call are the same bytes; the matrix values of a
 *                            regular row are written once by one lane and depend neither on the z-chunk length nor on
 *                            PFM_OVERLAY3_CONCURRENT.  NOT PROMISED: the rows of the general family (hanging, parent,
 *                            mixed-level rows and their neighbours) agree between the two calls to rounding only (measured:
 *                            see profiles/split_lattice_jacobian_levels/README.md).  A cell next to the seam is evaluated by
 *                            both families, each with its own tr E: where tr E is zero up to rounding the matrix is not
 *                            determined, as above.  On a box or a sub-box this route is PFM_SPLIT_ROUTE_LATTICE_JACOBIAN
 *                            byte for byte; under model 0 or 1, in 2-D (refused as every lattice route), on path 0 and with
 *                            the split off it acts as that route does.  An overlay under PFM_SPLIT_ROUTE_LATTICE_JACOBIAN
 *                            or _ALL keeps the general family for its full assembly, as before.  COST: this route is NOT
 *                            faster than the general route on an overlay -- measured on the block-refined 84^3 mesh (1.1e6
 *                            cells, 93 % regular rows) 22.4 ms per full assembly against 13.7 ms, above it in every round
 *                            (profiles/split_lattice_jacobian_levels/README.md).  It is opt-in for the residual guarantee.
 *   PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS  (= 1 | 2 | 4 | 8) the same with the residual-only calls of
 *                            PFM_SPLIT_ROUTE_LATTICE_ANY.  Every other value with bit 8 (8, 9, 10, 11, 12, 14) is refused
 *                            with PFM_ERR_BAD_ARG.
 *   PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE  (= 1 | 4 | 16) PFM_SPLIT_ROUTE_LATTICE_JACOBIAN with the law evaluated only where
 *                            it differs from the unsplit one.  Under PFM_SPLIT_VOLDEV the law is the unsplit law wherever
 *                            tr E >= 0 (h = 1: the tangent weight is lambda g, sigma+ = sigma).  The FULL assembly of a 3-D box
 *                            or partitioned sub-box becomes, on the context's stream: residual_pde from
 *                            k_cart_residual3<false, true> exactly as under route 5; k_cart_split3_mark, a lane per lattice
 *                            cell, writes one byte per cell (1: some q-point has h(tr E) = 0, by the trace statement of
 *                            k_cart_split3_jac), flags the tile-chunks that own a vertex of such a cell and counts them;
 *                            the unsplit k_cart_uu3 and k_cart_phi4 (the plan of the same parameters with
 *                            decompose_stress_matrix = 0, no residual rows, not paired) write every row; the sparse form
 *                            of k_cart_split3_jac leaves a tile-chunk without a flag at once, passes by every node none of
 *                            whose (up to) eight cells has its byte set, and writes the four rows of the other nodes again
 *                            as under route 5.  No compaction pass, no host read-back.  In an overlapped assembly all of
 *                            this but the residual kernel runs whole in the second half.  PROMISED: a row of a node that
 *                            is a vertex of a local cell with a q-point where the device's tr E < 0 holds, in all four
 *                            blocks, the bytes of route 5 on the same context and state, for any z-chunk length; every
 *                            other row holds what those unsplit kernels wrote; residual_pde is route 5's bytes (and the
 *                            residual-only call's); the assembly is bitwise reproducible run to run and on a fresh
 *                            context; the (u,phi) block holds exact zeros.  NOT PROMISED: the bytes of the untouched rows
 *                            against an unsplit assembly that runs other instantiations (the pair with residual rows:
 *                            equal to rounding), against the general route, or between a box and its sub-boxes (to
 *                            rounding); and, as everywhere under this law, where tr E is zero up to rounding the matrix is
 *                            not determined.  Residual-only calls are those of route 5 bit for bit.  Under model 0 or 1,
 *                            with the split off, on path 0 and on the level lattices of an overlay the route acts as route
 *                            5 does (an overlay context keeps the general family for its full assembly).  COST: the
 *                            route pays the unsplit kernels and the mark kernel everywhere and the split kernel where
 *                            cells are compressed.  Measured per full assembly at 1e6 hexes against route 5's 10.2 ms
 *                            (profiles/split_lattice_jacobian_sparse/README.md): 1.34 ms with no compressed cell, 4.92 ms
 *                            with a slab of 5 % of the cells compressed, below route 5 in every round -- and 11.49 ms,
 *                            1.13 times route 5 and above it in every round, where nearly every cell has a compressed
 *                            q-point: on such a state it is SLOWER than route 5.
 *   PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE  (= 1 | 2 | 4 | 16) the same with the residual-only calls of
 *                            PFM_SPLIT_ROUTE_LATTICE_ANY.  Every other value with bit 16 (16-20, 22, 24-31: bit 16 without
 *                            the Jacobian route, or together with bit 8) is refused with PFM_ERR_BAD_ARG.
 *   PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE  (= 1 | 4 | 8 | 16 | 32) PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS with the law
 *                            evaluated only where it differs from the unsplit one, on the level lattices of a 3-D overlay
 *                            too (bit 32: valid only together with bits 8 and 16).  The FULL assembly of a 3-D overlay under
 *                            PFM_SPLIT_VOLDEV with the split on, for every scheme, both layouts, per-cell Lame coefficients
 *                            and any decompose_stress_matrix / decompose_stress_rhs weights, becomes per level lattice, on
 *                            that level's stream (the context's, or its own under PFM_OVERLAY3_CONCURRENT=1):
 *                            k_cart_residual3<false, true> writes residual_pde of the regular rows exactly as under route
 *                            13; the level form of k_cart_split3_mark, a lane per cell of the level lattice, takes the cells
 *                            whose eight vertices all exist on that level, writes one byte per cell (1: some q-point has
 *                            h(tr E) = 0, by the trace statement of k_cart_split3_jac), flags the tile-chunks that own a
 *                            regular row among the cell's vertices and counts the cell if its lowest vertex is a regular row
 *                            of this rank (route 13's rule); the unsplit k_cart_uu3 and k_cart_phi4 of the level (the plan
 *                            of the same parameters with decompose_stress_matrix = 0, no residual rows) write every regular
 *                            row; k_cart_split3_jac<NCOL, true, true> leaves a tile-chunk without a flag at once, passes by
 *                            every node that is no regular row or none of whose (up to) eight level cells has its byte set,
 *                            and writes the four rows of the other nodes again as under route 13.  The general family runs
 *                            exactly as under route 13.  No compaction pass, no host read-back, no floating-point atomics in
 *                            these kernels.  PROMISED: a regular row whose node is a vertex of a level cell with a q-point
 *                            where the device's tr E < 0 holds route 13's bytes in all four blocks, for any z-chunk length;
 *                            every non-regular row holds route 13's bytes as long as pfm_ctx_hanging_info out[4] is 0;
 *                            residual_pde is route 13's bytes on every row, and on the regular rows the residual-only
 *                            call's; every other regular row holds what the unsplit level kernels wrote; the (u,phi) block
 *                            holds exact zeros; the assembly is bitwise reproducible run to run, on a fresh context and
 *                            under PFM_OVERLAY3_CONCURRENT=1.  NOT PROMISED: the untouched rows against an unsplit overlay
 *                            assembly that runs other instantiations (homogeneous material in the linear scheme: residual
 *                            rows in the Jacobian kernels; or time step 0 under the monolithic scheme, which drops the
 *                            penalty term: with per-cell Lame coefficients and decompose_stress_matrix = 0 on the same
 *                            context they are the same bytes), the untouched rows against the general route, and, as
 *                            everywhere under this law, the matrix where tr E is zero up to rounding.  On a box or
 *                            partitioned sub-box the route is PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE byte for byte (values,
 *                            residual_pde, both info calls, both halves of the overlapped assembly); with the split off,
 *                            under model 0 or 1 and on path 0 it acts as route 13, bit for bit; residual-only calls are
 *                            those of route 13.  An overlay under PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE or _ALL_SPARSE
 *                            keeps the general family for its full assembly, as before.  COST: per level the unsplit
 *                            kernels and the mark kernel everywhere, the split kernel where cells are compressed, plus the
 *                            general-family part of route 13.  Measured per full assembly on the block-refined 84^3 mesh
 *                            (1.1e6 cells, 93 % regular rows) in one process against the general route's 13.6-13.8 ms,
 *                            route 13's 22.2 ms and the unsplit overlay assembly's 3.76 ms
 *                            (profiles/split_lattice_jacobian_levels_sparse/README.md): 4.10 ms with no compressed cell
 *                            and 8.92 ms with a slab of 6.6 % of the cells compressed (8.1 % of the regular rows
 *                            recomputed), below both routes in every round -- and 25.6 ms, 1.88 times the general route
 *                            and 1.15 times route 13, above both in every round, where nearly every regular row touches a
 *                            compressed cell: on such a state it is SLOWER than the general route.
 *   PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE  (= 1 | 2 | 4 | 8 | 16 | 32) the same with the residual-only calls of
 *                            PFM_SPLIT_ROUTE_LATTICE_ANY (route 15's); on a box PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE.  Every
 *                            other value with bit 32 (32-60, 62, and anything above 63) is refused with PFM_ERR_BAD_ARG.
 * May be called at any time on a living context: the next assembly follows it.  An unknown route: PFM_ERR_BAD_ARG.
 * Any route but PFM_SPLIT_ROUTE_GENERAL on a 2-D context: PFM_ERR_UNSUPPORTED.  PFM_SPLIT_ROUTE_LATTICE with model 0 or 1 is
 * accepted and has no effect.
 * pfm_ctx_split_route: the route set and, lattice_residual, whether a residual-only assembly with the current parameters,
 * model and forced path would run its law, either one, on the row-owner kernels (0 before pfm_set_params); either pointer
 * may be null.
 * pfm_ctx_split_route_info: answered from the plan of such assemblies.  out[0] the route; out[1] whether a residual-only
 * assembly would run its law on the row-owner kernels (what pfm_ctx_split_route answers); out[2] whether a full assembly
 * would (0 before pfm_set_params); out[3] the number of owned cells (cells whose lowest vertex this rank owns) with at least
 * one compressed q-point, h(tr E) = 0, as counted by k_cart_split3_jac in the last full assembly of this context -- -1 when
 * that assembly did not run on that kernel or none has run.  On a 3-D overlay under the _LEVELS routes out[2] is 1 and
 * out[3] covers the cells of the level kernels only: the cells whose lowest vertex is a regular row, summed over the levels
 * (the cells of the general family are not counted).  Reading out[3] waits for the context's stream.  Under the _SPARSE
 * routes out[2] is 1 and out[3] is the count of k_cart_split3_mark: on any state the number route 5 reports (on an overlay
 * under the _LEVELS_SPARSE routes: the number route 13 reports, summed over the levels).
 * pfm_ctx_split_sparse_info: out[0] whether a full assembly with the current parameters, model, route and forced path would
 * run sparse (0 before pfm_set_params); out[1] the nodes whose rows the sparse form of k_cart_split3_jac recomputed in the
 * last full assembly of this context, -1 when that one did not run sparse or none has run; out[2] the tile-chunks flagged
 * in that assembly (-1 likewise); out[3] the tile-chunks of the grid (of the plan of out[0]; 0 when out[0] is 0).  Reading
 * out[1] and out[2] waits for the context's stream.  On a 3-D overlay under the _LEVELS_SPARSE routes out[0] is 1 when a full
 * assembly would run sparse on the level lattices, out[1] the regular rows recomputed and out[2] the tile-chunks flagged in
 * the last full assembly, both summed over the levels, out[3] the tile-chunks of all level grids; under the _SPARSE routes
 * out[0] stays 0 there. */
enum
{
  PFM_SPLIT_ROUTE_GENERAL = 0,
  PFM_SPLIT_ROUTE_LATTICE = 1,
  PFM_SPLIT_ROUTE_LATTICE_ANY = 3,
  PFM_SPLIT_ROUTE_LATTICE_JACOBIAN = 5,
  PFM_SPLIT_ROUTE_LATTICE_ALL = 7,
  PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS = 13,
  PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS = 15,
  PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE = 21,
  PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE = 23,
  PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE = 61,
  PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE = 63
};
int pfm_set_split_route(pfm_ctx *ctx, int route);
int pfm_ctx_split_route(const pfm_ctx *ctx, int *route, int *lattice_residual);
int pfm_ctx_split_route_info(const pfm_ctx *ctx, int64_t out[4]);
int pfm_ctx_split_sparse_info(const pfm_ctx *ctx, int64_t out[4]);
/* How the cells at hanging vertices of a general mesh (2-D or 3-D, with or without a cartesian overlay) reach the outputs.
 *   PFM_HANGING_MODE_DEFAULT  what every context did before this call existed, bit for bit: 3-D unsplit and model 3 write
 *                             K' = C^T K C, R' = C^T R and their placeholder diagonals to per-cell scratch, and an ordered
 *                             gather adds them row by row in list order (no FP64 atomics, bitwise reproducible); 3-D model 1
 *                             and every 2-D mesh run them as a last class with atomic adds, the cells of the plain classes
 *                             that share a node with them as well.  PFM_HANGING_ATOMIC=1 and PFM_HANGING_COLOURED=1 at
 *                             context creation are honoured as before.
 *   PFM_HANGING_MODE_GATHER   scratch + ordered gather wherever a form exists: 2-D (Jacobian and residual-only, split and
 *                             unsplit, both layouts, with and without the patch overlay) and 3-D under every law, the
 *                             spectral one and its route-3 overlay residual included.  The plain classes then run without
 *                             atomics.  Such an assembly is bitwise reproducible run to run and context to context.
 *   PFM_HANGING_MODE_ATOMIC   the atomic class everywhere: what PFM_HANGING_ATOMIC=1 selects at creation, settable on a
 *                             living context for A/B runs.
 * May be called at any time on a living context: the next assembly follows it.  An unknown mode: PFM_ERR_BAD_ARG (the mode
 * stays).  PFM_HANGING_MODE_GATHER on a context created under PFM_HANGING_COLOURED=1: PFM_ERR_UNSUPPORTED.  On a context
 * without hanging nodes every mode is accepted and has no effect.  Silent fallbacks, as in 3-D before: a cell with more than
 * 16 constraint-resolved nodes makes the context keep its atomic class in every mode (a quad has at most 16 by
 * construction); after a colour overflow (a node of more than 62 cells) the plain classes keep their atomic adds.
 * pfm_ctx_hanging_info reports what actually happens: *mode the mode set; out[0] the number of cells at hanging vertices;
 * out[1] 1 if the next assembly with the current parameters, model, route and forced path sends them through the gather;
 * out[2] the rows of the gather tables (0 until the first such assembly builds them); out[3] the device bytes held for the
 * tables and the scratch (counted in pfm_ctx_device_bytes); out[4] 1 if that assembly would issue any floating-point atomic
 * add (atomic class, ring cells, colour overflow) -- the bitwise promise holds exactly when it is 0.  out[1] and out[4] are
 * 0 before pfm_set_params; either pointer may be null. */
enum
{
  PFM_HANGING_MODE_DEFAULT = 0,
  PFM_HANGING_MODE_GATHER = 1,
  PFM_HANGING_MODE_ATOMIC = 2
};
int pfm_set_hanging_mode(pfm_ctx *ctx, int mode);
int pfm_ctx_hanging_info(const pfm_ctx *ctx, int *mode, int64_t out[5]);
/* constraints_update minus the hanging nodes: one byte per local node, bit c set <=> dof
 * (node, c) has a homogeneous line (Dirichlet from set_newton_bc cracks.cc:2711-2714, or
 * active set cracks.cc:2878-2879).  Call whenever constraints_update is rebuilt. */
int pfm_set_constraints(pfm_ctx *ctx, const uint8_t *node_flags /* host, [n_nodes] */);

/* -- matrix pattern ------------------------------------------------------------------- */
int pfm_pattern_size(const pfm_ctx *ctx, int block, int64_t *n_rows, int64_t *nnz);
/* host outputs: rowptr[n_rows+1], colind[nnz]: the pattern the value arrays of pfm_assemble_device follow.  After
 * pfm_ctx_create the columns of every row ascend by local id (owned columns first, ghost columns last): the layout of
 * a host CSR sorted by local column index, e.g. an Epetra_CrsMatrix after FillComplete with optimised storage. */
int pfm_pattern_get(const pfm_ctx *ctx, int block, int64_t *rowptr, int32_t *colind);
/* Bind the HOST's pattern of `block` (make_sparsity_pattern + reinit, cracks.cc:1644-1654; the arrays
 * Epetra_CrsMatrix::ExtractCrsDataPointers returns): from now on the value arrays handed to the assembly are laid
 * out exactly like the host's values[] -- the library borrows the host's CSR, it does not dictate one.  The arrays are
 * read during the call only.  Requirements (checked, PFM_ERR_BAD_ARG otherwise): same rows and the same set of
 * columns per row as pfm_pattern_get (the node graph of the constraint-resolved mesh, full component coupling); within a
 * row the entries of one neighbour node adjacent with ascending component.  Any order of the neighbour nodes is
 * accepted, but all blocks must use the same one (PFM_ERR_UNSUPPORTED).  Binding a pattern that already has the
 * library's order is a pure check.  _i32: 32-bit row pointers (Epetra's int offsets). */
int pfm_pattern_bind(pfm_ctx *ctx, int block, const int64_t *rowptr, const int32_t *colind);
int pfm_pattern_bind_i32(pfm_ctx *ctx, int block, const int32_t *rowptr, const int32_t *colind);

/* -- state: the three vectors read at cracks.cc:2147-2154 ----------------------------- */
/* Scatter the OWNED dofs of solution / old_solution / old_old_solution (dof vectors in the
 * context's layout; host pointers if on_device == 0, device pointers otherwise) into the
 * context's node arrays.  Only the phase-field block of old / old_old is read
 * (cracks.cc:2229, 2232). */
int pfm_state_set(pfm_ctx *ctx, const double *sol, const double *old, const double *oldold,
                  int on_device);
/* The same for `solution` alone: old / old_old keep the values of the last pfm_state_set.  This is the call of the
 * line search (cracks.cc:2942-2957: solution += delta; assemble_nl_residual(), up to max_no_line_search_steps times per
 * Newton step while old_solution / old_old_solution do not change) and of every Newton iteration after the first of a
 * time step: a third of the scatter traffic of pfm_state_set.  Ghost values of solution still come from
 * pfm_halo_exchange. */
int pfm_state_set_solution(pfm_ctx *ctx, const double *sol, int on_device);
/* Ghost import (cracks.cc:2147-2154) as pack -> RCCL send/recv -> unpack; the exchange itself is
 * done by the host side between the two calls.  Registration copies the lists.
 * send_nodes: owned nodes whose values a peer needs; recv_nodes: ghost nodes a peer owns.
 * A packed node record is PFM_HALO_DOUBLES_PER_NODE(dim) doubles: u[dim], phi, phi_old, phi_oldold. */
#define PFM_HALO_DOUBLES_PER_NODE(dim) ((dim) + 3)
int pfm_halo_register(pfm_ctx *ctx, int n_peers, const int64_t *send_ptr, const int32_t *send_nodes,
                      const int64_t *recv_ptr, const int32_t *recv_nodes);
int pfm_halo_pack(pfm_ctx *ctx, int peer, double *d_buf);         /* device buffer */
int pfm_halo_unpack(pfm_ctx *ctx, int peer, const double *d_buf); /* device buffer */
/* All peers with one launch: d_buf_all holds the messages back to back in peer order, the message of peer k starts at
 * PFM_HALO_DOUBLES_PER_NODE(dim) * send_ptr[k] (pack) resp. * recv_ptr[k] (unpack) and has the same layout as the
 * per-peer calls produce. */
int pfm_halo_pack_all(pfm_ctx *ctx, double *d_buf_all);
int pfm_halo_unpack_all(pfm_ctx *ctx, const double *d_buf_all);

/* The whole ghost import inside the library, for hosts without torch (the deal.II application): RCCL point-to-point
 * over xGMI in place of the Trilinos/MPI import of cracks.cc:2147-2154.
 *   pfm_comm_unique_id   ncclGetUniqueId on one rank; the host broadcasts the bytes (MPI_Bcast in the reference's world)
 *   pfm_comm_create      ncclCommInitRank: collective over the n_ranks processes, one GPU each
 *   pfm_halo_exchange    pack (one launch) -> ncclGroupStart, ncclSend/ncclRecv per peer, ncclGroupEnd -> unpack (one
 *                        launch), all asynchronous on the context's stream, into buffers the context owns;
 *                        peer_ranks[k] = communicator rank of peer k of pfm_halo_register.  `comm` is a handle made
 *                        by pfm_comm_create, or by pfm_comm_wrap around the host's own ncclComm_t.  Collective: every
 *                        rank of the communicator that is somebody's peer must call it.
 *                        A raw ncclComm_t is NOT a handle: it is refused with PFM_ERR_BAD_ARG (the handles carry a tag).
 * Error path: a failed exchange on a communicator made by pfm_comm_create aborts it (ncclCommAbort: peers error out
 * instead of waiting for a message that never comes).  A communicator adopted with pfm_comm_wrap belongs to the host: it
 * is neither aborted nor destroyed by the library -- the handle is disabled and the host decides (abort or destroy its
 * ncclComm_t as usual).  Either way the HANDLE stays valid: pfm_comm_aborted() reports 1, every further exchange on it
 * returns PFM_ERR_COMM, and pfm_comm_destroy() only frees the handle then (no double free). */
#define PFM_COMM_ID_BYTES 128
int pfm_comm_unique_id(uint8_t id[PFM_COMM_ID_BYTES]);
int pfm_comm_create(void **comm, const uint8_t id[PFM_COMM_ID_BYTES], int n_ranks, int rank, int device);
int pfm_comm_wrap(void **comm, void *nccl_comm /* the host's ncclComm_t; not destroyed by pfm_comm_destroy */);
int pfm_comm_destroy(void *comm);
int pfm_comm_aborted(const void *comm); /* 1 after a failed exchange aborted the communicator, else 0 */
/* what RCCL itself reports for the communicator behind a handle: ncclCommCount, ncclCommUserRank (-1 where the loaded RCCL has
 * no such entry point) and ncclGetVersion -- diagnostics for multi-GPU records; any of the pointers may be NULL */
int pfm_comm_info(const void *comm, int *n_ranks, int *rank, int *rccl_version);
int pfm_halo_exchange(pfm_ctx *ctx, void *comm, const int *peer_ranks /* host, [n_peers] */);
/* pfm_halo_exchange + pfm_assemble_device with the ghost import HIDDEN behind cell work: after pfm_state_set the exchange
 * runs on a second stream of the context while the tiles that read no ghost node are assembled; the rest follows when the
 * import has landed.  Same results as the two calls in sequence (bit for bit on uniform boxes); same collective rule as
 * pfm_halo_exchange.  Declared here, next to the call it replaces; arguments as pfm_assemble_device. */
int pfm_assemble_overlapped(pfm_ctx *ctx, void *comm, const int *peer_ranks, int residual_only, double *const *d_values,
                            double *d_res_pde, double *d_res_tot);

/* -- the hot path --------------------------------------------------------------------- */
/* assemble_system(residual_only) on the current state.  Output pointers are DEVICE
 * pointers; the call is asynchronous on the context's stream.
 *   residual_only != 0: residual_pde (through constraints_update) and residual_total
 *     (through constraints_hanging_nodes for the active-set solver, constraints_update
 *     otherwise; cracks.cc:2440-2456) are zeroed and assembled; values is ignored.
 *   residual_only == 0: values[block] and residual_pde are zeroed and assembled
 *     (cracks.cc:2457-2464); residual_total is ignored.
 * Rows of ghost nodes are never written: each rank computes its owned rows completely
 * (it also integrates its ghost-layer cells), so no reverse exchange (compress(add),
 * cracks.cc:2470-2475) is needed. */
int pfm_assemble_device(pfm_ctx *ctx, int residual_only, double *const *d_values /* [n_blocks] */,
                        double *d_residual_pde, double *d_residual_total);
/* assemble_nl_residual() after `solution` alone changed -- the call of the line search (cracks.cc:2942-2957: solution +=
 * delta; assemble_nl_residual(), up to max_no_line_search_steps times per Newton step; cracks.cc:2507-2512):
 * = pfm_state_set_solution(d_solution, on_device = 1) + pfm_assemble_device(residual_only = 1) in one call.  On a
 * single-rank 3-D box the residual kernel reads d_solution itself and the scatter launch disappears.  Ranks with halo
 * peers import ghosts between the two steps and keep calling them separately (PFM_ERR_BAD_ARG here). */
int pfm_assemble_nl_residual_device(pfm_ctx *ctx, const double *d_solution, double *d_residual_pde, double *d_residual_total);
/* Blocks until the stream is idle and returns the deferred status of the launches since
 * the last call (PFM_ERR_NOT_ORTHOGONAL, PFM_ERR_HIP, ...). */
int pfm_sync_status(pfm_ctx *ctx);

/* On request: scan n doubles of a device array (an assembled residual or value block) for NaN / Inf.  Returns
 * PFM_ERR_NONFINITE if there is one, else whatever pfm_sync_status() would return.  The assembly itself never checks:
 * like the reference it lets IEEE specials propagate (e.g. the stress split at diagonal or zero strain,
 * cracks.cc:1982-2006). */
int pfm_check_finite(pfm_ctx *ctx, const double *d_data, int64_t n);

/* Host-visible outputs (cracks.cc:2754, 2770, 2918: the caller hands system_pde_matrix to Trilinos right after the call).
 *   pfm_host_register    page-locks a host array the host-pointer entry points read or write at every call -- the value
 *                        arrays of the Epetra_CrsMatrix blocks (Epetra_CrsMatrix::ExtractCrsDataPointers), the owned parts of
 *                        the vectors -- so that their transfers run as DMA at the link rate instead of through the runtime's
 *                        pageable path.  The array stays the caller's; it must be unregistered (pfm_host_unregister, NULL =
 *                        all; pfm_ctx_destroy does it too) BEFORE it is freed or reallocated (setup_system after refine_mesh).
 *                        PFM_ERR_HIP if the pages cannot be locked (ulimit): the array simply stays pageable.
 *   pfm_values_to_host   matrix values of the last pfm_assemble_device -> h_values[block], synchronous.  With the 2x2 block
 *                        layout the (u,phi) block is identically zero (trial phase-field dofs do not enter the displacement
 *                        rows, cracks.cc:2333-2337; the placeholders of constrained rows sit on the diagonals of (u,u) and
 *                        (phi,phi)): 3/16 of the bytes.  If h_values[1] is a REGISTERED array it is cleared once by host
 *                        threads and never transferred -- the library assumes nobody else writes the matrix values between
 *                        assemblies (the reference only fills them through assemble_system); an unregistered array is copied
 *                        like the other blocks.  Blocks 2, 3 travel on a second stream next to block 0.
 * pfm_assemble = pfm_state_set + pfm_assemble_device + these copies + pfm_sync_status: the exact call shape of the
 * reference (outputs complete in host memory on return, cracks.cc:2791-2794, 2918).  Single-rank only (no ghosts). */
int pfm_host_register(pfm_ctx *ctx, void *host_array, int64_t bytes);
int pfm_host_unregister(pfm_ctx *ctx, void *host_array /* NULL: every array of this context */);
int pfm_values_to_host(pfm_ctx *ctx, double *const *d_values /* [n_blocks] */, double *const *h_values /* [n_blocks] */);
int pfm_assemble(pfm_ctx *ctx, const double *sol, const double *old, const double *oldold,
                 int residual_only, double *const *values, double *residual_pde,
                 double *residual_total);

/* A kept (u,phi) block (4-block layout only).  The block is identically zero on every path of the library and of the
 * reference (cracks.cc:2333-2337), yet it is 3/16 of the matrix values and 18.5 % of every byte a blocked 3-D Jacobian
 * assembly writes.  With a promise from the caller the library writes it once and never again.
 *   pfm_values_keep_up_block   clears block_nnz(1) doubles at d_values_up to +0.0 (on the context's stream, complete on
 *                              return) and remembers the pointer.  From then on the caller promises that nothing but this
 *                              library writes that array; in turn every pfm_assemble_device / pfm_assemble_overlapped whose
 *                              d_values[1] EQUALS that pointer may leave the block untouched.  A call with any other
 *                              d_values[1] behaves as without a promise and leaves the promise in place.  One promise per
 *                              context: another pointer replaces it, the same pointer again clears the array again.  NULL
 *                              withdraws it.  PFM_ERR_BAD_ARG for the interleaved layout and for a non-NULL pointer when
 *                              block_nnz(1) == 0.  The array stays the caller's; the promise must be withdrawn (NULL here;
 *                              pfm_ctx_destroy does it too) BEFORE the array is freed or reallocated (setup_system after
 *                              refine_mesh).  It survives pfm_set_params, pfm_set_constraints, pfm_pattern_bind*,
 *                              pfm_set_split_model / _route, pfm_set_hanging_mode, pfm_ctx_force_path / _phase / _zchunk and
 *                              pfm_ctx_set_stream.  PFM_NO_KEEP_UP_BLOCK=1 (read per call): the promise is ignored and every
 *                              path writes the block.
 *   pfm_values_up_block_kept   the kept pointer, NULL if there is none.
 * pfm_assemble (host pointers) keeps the block of its own staging arrays itself, without a promise from anyone. */
int pfm_values_keep_up_block(pfm_ctx *ctx, double *d_values_up /* NULL: withdraw */);
int pfm_values_up_block_kept(const pfm_ctx *ctx, const double **d_values_up);

/* A kept (u,u) block (4-block layout only).  In the quasi-monolithic scheme without the penalty term and without a stress
 * split (every Sneddon and Miehe parameter file of the reference) the (u,u) block is a function of old_solution,
 * old_old_solution, the displacement constraints and the parameters -- not of `solution` (cracks.cc:2262-2277, 2353-2364,
 * 4275) -- so every Newton iteration of a time step after the first rewrites the same values: 9/16 of the matrix.
 *   pfm_values_keep_uu_block   remembers the pointer; nothing is cleared or written.  The caller promises that nothing but
 *                              this library writes that array.  In turn a pfm_assemble_device / pfm_assemble_overlapped
 *                              whose d_values[0] EQUALS that pointer leaves the block alone when it provably holds the
 *                              current values: the library raises a device word whenever an input of the block changes
 *                              (the promise itself, pfm_set_params with other bytes, pfm_set_constraints with another
 *                              displacement bit, pfm_pattern_bind*, pfm_set_split_model / _route, pfm_ctx_force_path /
 *                              _zchunk, pfm_state_set with another bit pattern of old or oldold at any owned node, any
 *                              assembly that wrote the array on another path), the (u,u) kernel reads it on the device and
 *                              the call stays asynchronous.  The promise takes effect only on the two-stream pair of a
 *                              3-D box: linear scheme, kappa < 0.5, homogeneous material, whole assembly, no level lattice, a
 *                              context without ghost nodes or peers, none of PFM_RES_KERNEL / PFM_JAC_SEQUENTIAL / the phase
 *                              clocks.  Everywhere else it is accepted and ignored and the block is written at every
 *                              assembly.  Under the promise, where it takes effect, the displacement rows of residual_pde
 *                              come from the quadrature kernel in EVERY assembly, written or kept: they are the rows
 *                              PFM_RES_KERNEL=1 gives, bit for bit, equal from one assembly to the next, within the parity
 *                              bar of the reference, and not bit-equal to the rows the Jacobian kernel derives from its
 *                              matrix rows without the promise.  The four value blocks keep their bits.  A call with any
 *                              other d_values[0] behaves as without a promise and leaves it in place.  One promise per
 *                              context; NULL withdraws it (pfm_ctx_destroy does it too) and must do so BEFORE the array is
 *                              freed or reallocated.  PFM_ERR_BAD_ARG for the interleaved layout and for a non-NULL pointer
 *                              when block_nnz(0) == 0.  PFM_NO_KEEP_UU_BLOCK=1 (read per call): ignored everywhere.
 *   pfm_values_uu_block_kept   the kept pointer, NULL if there is none.
 * pfm_assemble (host pointers) is unchanged: its cost is the copy to the host. */
int pfm_values_keep_uu_block(pfm_ctx *ctx, double *d_values_uu /* NULL: withdraw */);
int pfm_values_uu_block_kept(const pfm_ctx *ctx, const double **d_values_uu);

/* Delta transfer of the matrix values ("Delta transfer"): within a time step most of the Jacobian does not
 * change between Newton iterations (without the stress split the displacement rows depend on the lagged phase field
 * only), and the library finds out itself which values did.
 *
 * Like pfm_values_to_host, but only chunks of d_values[b] whose BITS differ from what this function last left in
 * h_values[b] are transferred.  On return h_values[b][i] has the bit pattern of d_values[b][i] for every i, provided the
 * host has not written h_values[b] since the previous call on this context (the assumption pfm_values_to_host already
 * makes for a registered (u,phi) array).  Synchronous; ordered behind earlier work on the context's stream.
 *   comparison     on the 64-bit patterns, never a floating-point compare: -0.0 and 0.0 differ, two NaNs with different
 *                  payloads differ, identical NaNs are equal.
 *   state          the library keeps a device copy (the "shadow") of what the host holds for each block: exact, not a
 *                  hash.  Allocated at the first call, counted in pfm_ctx_device_bytes, freed by pfm_ctx_destroy.  If it
 *                  (or the staging buffers) cannot be allocated the call returns PFM_ERR_NOMEM with the host arrays
 *                  untouched; the caller falls back to pfm_values_to_host.
 *   host pointers  h_values[b] is remembered per block; another pointer than last time ships all of that block.
 *   invalidation   pfm_pattern_bind*, pfm_values_delta_reset, pfm_values_delta_config, pfm_host_unregister of a
 *                  remembered array (or of all) and any error inside a delta call mark the state invalid: the next call
 *                  ships everything.
 *   sizes          1 block or 4, blocks with nnz == 0, blocks shorter than a chunk, a short last chunk, host arrays that
 *                  are only 8-byte aligned, registered or pageable.  Per rank; nothing collective.
 *   (u,phi)        in the 4-block layout a REGISTERED h_values[1] is cleared on the host instead of shipped when all of it
 *                  is due (once per registration, and again after pfm_values_delta_reset); it is compared like the other
 *                  blocks all the same, so a device block that is not all +0.0 still arrives bit for bit.
 * Each block is worked through in slabs: compare (one wave per chunk; a chunk that differs is copied to the shadow),
 * ordered scan of the flags, then the slab goes directly (d_values -> h_values, when most of its chunks changed) or packed
 * (changed chunks + their index list -> page-locked staging of the context -> memcpy per chunk by host threads).
 * stats (may be NULL): [0] bytes moved over the link (payload + chunk lists; not the 8-byte count word per slab),
 * [1] bytes of all blocks, [2] changed chunks, [3] chunks, [4] slabs shipped directly, [5] slabs shipped packed,
 * [6 + b] changed chunks of block b (b < 4). */
int pfm_values_to_host_delta(pfm_ctx *ctx, double *const *d_values, double *const *h_values, int64_t stats[10]);
/* forget what the host holds: the next delta call ships everything (the host zeroed or reallocated its arrays) */
int pfm_values_delta_reset(pfm_ctx *ctx);
/* tests and tuning, like pfm_ctx_force_zchunk: chunk_bytes a power of two >= 64, slab_bytes a multiple of chunk_bytes,
 * 0 = default; implies a reset.  Anything else PFM_ERR_BAD_ARG. */
int pfm_values_delta_config(pfm_ctx *ctx, int64_t chunk_bytes, int64_t slab_bytes);
/* out[0] chunk bytes, [1] slab bytes, [2] device bytes held for the feature, [3] 1 if the next call can skip anything */
int pfm_values_delta_info(const pfm_ctx *ctx, int64_t out[4]);

/* -- measurement ---------------------------------------------------------------------- */
/* When enabled, every pfm_assemble_device() brackets its kernel group (output zeroing where
 * the kernel family needs it, residual and Jacobian kernels; not the state scatter, which is
 * pfm_state_set_device) with HIP events on the context's stream;
 * pfm_kernel_time_ms() synchronises, returns the mean duration of the launches recorded
 * since the last call and resets the record. */
int pfm_timing_enable(pfm_ctx *ctx, int on);
int pfm_kernel_time_ms(pfm_ctx *ctx, double *mean_ms, int *n_launches);
/* The individual durations (for a median): the first min(capacity, recorded) ones; *n_launches = recorded.  Does not
 * reset the record (pfm_kernel_time_ms / pfm_timing_enable do). */
int pfm_kernel_times_ms(pfm_ctx *ctx, double *ms, int capacity, int *n_launches);

/* -- introspection -------------------------------------------------------------------- */
/* which kernel family the context selected: 0 = general (any Q1 mesh), 1 = cartesian (uniform box; its 2-D stress-split runs
 * use the overlay below), 3 = general family + cartesian overlay: 2-D meshes with hanging nodes, slits, several refinement
 * levels -- the rows of regular lattice nodes are completed by one workgroup per 8 x 8 block of their level, the general
 * family keeps the cells that touch any other row.  pfm_ctx_force_path(0) selects the general family alone (A/B runs). */
int pfm_ctx_kernel_path(const pfm_ctx *ctx);
int pfm_ctx_force_path(pfm_ctx *ctx, int path);
/* composition of the overlay: rows written by the patch kernel / cells left to the general family (0 / all without it) */
int pfm_ctx_overlay_info(const pfm_ctx *ctx, int64_t *n_patch_rows, int64_t *n_general_cells);
/* measurement only: 1 / 2 make pfm_assemble_device run only the first / second half of pfm_assemble_overlapped (the work
 * that reads no ghost node / the rest), 0 restores the whole assembly: how much work hides the ghost import */
int pfm_ctx_force_phase(pfm_ctx *ctx, int phase);
/* tests and tuning: the z-chunk length of a marching kernel of the cartesian family, whose workgroups each march through
 * one chunk of node planes (2-D: node rows) -- kernel 0 = k_cart_uu3, 1 = k_cart_phi4, 2 = the 3-D residual kernels
 * (k_cart_residual3x / 3d / 3), 3 = k_cart_residual2m.  planes = 0 restores the default (PFM_UU_ZC, PFM_PHI_ZC, PFM_RES_ZC,
 * PFM_RES2_ZC if set, else the launch-time model); planes > 0 forces that length, clamped to the plane count of every
 * lattice the kernel runs on (the level lattices of a 3-D overlay included).  A null context, a kernel outside 0..3 or
 * planes < 0: PFM_ERR_BAD_ARG. */
int pfm_ctx_force_zchunk(pfm_ctx *ctx, int kernel, int planes);
/* the length the next launch of `kernel` over the context's own box uses, from the launchers' own helper (not in the
 * two halves of pfm_assemble_overlapped, where k_cart_uu3 marches single planes).  PFM_ERR_UNSUPPORTED: the context has
 * no box, or the kernel does not run in its dimension. */
int pfm_ctx_zchunk(const pfm_ctx *ctx, int kernel, int *planes);
int64_t pfm_ctx_device_bytes(const pfm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif

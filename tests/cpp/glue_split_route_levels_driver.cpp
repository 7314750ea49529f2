// tests/cpp/glue_split_route_levels_driver.cpp — TEST SCAFFOLDING like glue_split_route_jacobian_driver.cpp (the same set-up, the
// same outputs plus pfm_ctx_overlay_info), for the full assembly of a REFINED 3-D mesh under PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS / _ALL_LEVELS:
// PfmGlue::split_model and PfmGlue::split_route as given on the command line, on one rank
// (tests/test_gpu_glue_split_route_levels.py: PFM_SPLIT_VOLDEV with route 13 on the refined (8, 8, 8) block).
//
//   glue_split_route_levels_driver <dir> <model> <route> [<route> ...]
//       reads what glue_driver reads.  Per route r it builds a glue instance with its own "Trilinos" objects, runs a full
//       assembly and a residual-only one, and writes <dir>/sl_r<r>_val<2 row + col>.bin (the values of every block of
//       P.system_pde_matrix), _full.bin (P.system_pde_residual of the full assembly), _pde.bin (of the residual-only one) and
//       _info.bin (the four answers of pfm_ctx_split_route_info after the full assembly, pfm_ctx_kernel_path and the two answers
//       of pfm_ctx_overlay_info, as doubles)
#define main glue_driver_main
#include "glue_driver.cpp"
#undef main

#include <cstdlib>

// the set-up of glue_split_route_driver.cpp for the members of glue_driver.cpp's Problem
template <int dim>
static void setup_problem(Problem<dim> &P, const std::string &dir, std::istringstream meta /* behind dim */, int &blocked_out)
{
  constexpr int nv = 1 << dim;
  int blocked, n_nodes, n_cells, n_hanging, solver;
  meta >> blocked >> n_nodes >> n_cells >> n_hanging >> solver;
  blocked_out = blocked;
  P.direct_solver = !blocked;
  P.outer_solver = solver == 0 ? Problem<dim>::OuterSolverType::active_set : Problem<dim>::OuterSolverType::simple_monolithic;
  double pressure;
  int use_old, tsn;
  meta >> P.lame_coefficient_lambda >> P.lame_coefficient_mu >> P.G_c >> P.alpha_eps >> P.constant_k >> pressure >> P.alpha_biot >> P.gamma_penal >>
    P.timestep >> P.time >> P.old_timestep >> P.old_old_timestep >> P.decompose_stress_rhs >> P.decompose_stress_matrix >> tsn >> use_old;
  P.func_pressure.v = pressure;
  P.timestep_number = (unsigned int)tsn;
  P.use_old_timestep_pf = use_old != 0;
  const gidx n_u = (gidx)dim * n_nodes;
  auto dof_of = [&](int r, int comp) -> gidx {
    if (!blocked)
      return (gidx)((dim + 1) * r + comp);
    return comp < dim ? (gidx)(dim * r + comp) : n_u + (gidx)r;
  };
  const auto cells = read_bin<int32_t>(dir + "/cells.bin");
  const auto coords = read_bin<double>(dir + "/coords.bin");
  P.dof_handler.n_dofs_total = (gidx)(dim + 1) * n_nodes;
  P.dof_handler.cells.resize((size_t)n_cells);
  for (int c = 0; c < n_cells; ++c)
    for (int vtx = 0; vtx < nv; ++vtx)
      {
        const int r = cells[(size_t)c * nv + vtx];
        for (int comp = 0; comp <= dim; ++comp)
          P.dof_handler.cells[c].vdof[vtx][comp] = dof_of(r, comp);
        for (int d = 0; d < dim; ++d)
          P.dof_handler.cells[c].vert[vtx][d] = coords[(size_t)r * dim + d];
      }
  for (gidx g = 0; g < P.dof_handler.n_dofs_total; ++g)
    P.dof_handler.owned.idx.push_back(g);
  P.dof_handler.relevant = P.dof_handler.owned;
  if (n_hanging > 0)
    {
      const auto hn = read_bin<int32_t>(dir + "/hn_nodes.bin"), hp = read_bin<int32_t>(dir + "/hn_parents.bin");
      const auto ptr = read_bin<int64_t>(dir + "/hn_ptr.bin");
      const auto w = read_bin<double>(dir + "/hn_w.bin");
      for (int k = 0; k < n_hanging; ++k)
        for (int comp = 0; comp <= dim; ++comp)
          {
            AffineConstraints<double>::Line line;
            for (int64_t e = ptr[k]; e < ptr[k + 1]; ++e)
              line.emplace_back(dof_of(hp[e], comp), w[e]);
            P.constraints_hanging_nodes.lines[dof_of(hn[k], comp)] = line;
          }
    }
  P.constraints_update = P.constraints_hanging_nodes;
  {
    const auto fl = read_bin<uint8_t>(dir + "/con_update.bin");
    for (int r = 0; r < n_nodes; ++r)
      for (int comp = 0; comp <= dim; ++comp)
        if ((fl[r] >> comp) & 1u)
          P.constraints_update.lines[dof_of(r, comp)] = {};
  }
  const int nb1 = blocked ? 2 : 1;
  for (int r = 0; r < nb1; ++r)
    for (int c = 0; c < nb1; ++c)
      {
        Epetra_CrsMatrix &A = P.system_pde_matrix.block(r, c).trilinos_matrix();
        const std::string tag = std::to_string(2 * r + c);
        A.rowptr = read_bin<int>(dir + "/rowptr" + tag + ".bin");
        A.colind = read_bin<int>(dir + "/colind" + tag + ".bin");
        A.values.assign(A.colind.size(), 0.0);
        const long long ncol = blocked ? (c == 0 ? (long long)n_u : (long long)n_nodes) : (long long)(dim + 1) * n_nodes;
        A.colmap.gid.resize((size_t)ncol);
        for (long long g = 0; g < ncol; ++g)
          A.colmap.gid[(size_t)g] = g;
      }
}

static void set_vector(TrilinosWrappers::MPI::BlockVector &v, const std::vector<double> &x, size_t n_block0)
{
  v.block(0).v.assign(x.begin(), x.begin() + n_block0);
  v.block(1).v.assign(x.begin() + n_block0, x.end());
}
static std::vector<double> get_vector(const TrilinosWrappers::MPI::BlockVector &v)
{
  std::vector<double> x(v.block(0).begin(), v.block(0).end());
  x.insert(x.end(), v.block(1).begin(), v.block(1).end());
  return x;
}

template <int dim>
static void run_levels_route(const std::string &dir, const std::string &meta_text, int model, int route)
{
  const auto sol = read_bin<double>(dir + "/sol.bin"), old = read_bin<double>(dir + "/old.bin"), oldold = read_bin<double>(dir + "/oldold.bin");
  Problem<dim> P;
  int blocked = 0;
  std::istringstream meta(meta_text);
  int d;
  meta >> d;
  setup_problem<dim>(P, dir, std::move(meta), blocked);
  const size_t n0 = blocked ? sol.size() / (dim + 1) * dim : sol.size();
  set_vector(P.solution, sol, n0);
  set_vector(P.old_solution, old, n0);
  set_vector(P.old_old_solution, oldold, n0);
  const std::vector<double> zeros(sol.size(), 0.0);
  set_vector(P.system_pde_residual, zeros, n0);
  set_vector(P.system_total_residual, zeros, n0);
  pfm_glue_detail::PfmGlue<dim> glue;
  glue.split_model = model;
  glue.split_route = route;
  glue.rebuild(P);
  glue.assemble(P, /*residual_only=*/false);
  const std::vector<double> full = get_vector(P.system_pde_residual);
  int64_t info[4] = {-2, -2, -2, -2};
  if (pfm_ctx_split_route_info(glue.ctx, info) != PFM_OK)
    throw std::runtime_error("pfm_ctx_split_route_info");
  const std::string tag = dir + "/sl_r" + std::to_string(route);
  const int nb1 = blocked ? 2 : 1;
  for (int r = 0; r < nb1; ++r)
    for (int c = 0; c < nb1; ++c)
      {
        const Epetra_CrsMatrix &A = P.system_pde_matrix.block(r, c).trilinos_matrix();
        write_bin(tag + "_val" + std::to_string(2 * r + c) + ".bin", A.values.data(), A.values.size());
      }
  glue.assemble(P, /*residual_only=*/true);
  const std::vector<double> pde = get_vector(P.system_pde_residual);
  write_bin(tag + "_full.bin", full.data(), full.size());
  write_bin(tag + "_pde.bin", pde.data(), pde.size());
  int64_t rows = -1, general_cells = -1;
  if (pfm_ctx_overlay_info(glue.ctx, &rows, &general_cells) != PFM_OK)
    throw std::runtime_error("pfm_ctx_overlay_info");
  const double out[7] = {(double)info[0], (double)info[1], (double)info[2], (double)info[3], (double)pfm_ctx_kernel_path(glue.ctx), (double)rows,
                         (double)general_cells};
  write_bin(tag + "_info.bin", out, (size_t)7);
}

int main(int argc, char **argv)
{
  if (argc < 4)
    {
      std::fprintf(stderr, "usage: glue_split_route_levels_driver <dir> <model> <route> [<route> ...]\n");
      return 2;
    }
  try
    {
      const std::string dir = argv[1];
      std::ifstream f(dir + "/meta.txt");
      std::stringstream ss;
      ss << f.rdbuf();
      std::istringstream meta(ss.str());
      int dim;
      meta >> dim;
      if (dim != 3)
        throw std::runtime_error("the split route is a 3-D matter");
      for (int a = 3; a < argc; ++a)
        run_levels_route<3>(dir, ss.str(), std::atoi(argv[2]), std::atoi(argv[a]));
      std::printf("glue_split_route_levels_driver: OK\n");
      return 0;
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "glue_split_route_levels_driver: FAILED: %s\n", e.what());
      return 1;
    }
}

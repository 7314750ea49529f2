// tests/cpp/glue_hanging_mode_driver.cpp — TEST SCAFFOLDING like glue_driver.cpp (whose Problem and file helpers it reuses):
// PfmGlue::hanging_mode = PFM_HANGING_MODE_GATHER on one rank (tests/test_gpu_glue_hanging_mode.py).
//
//   glue_hanging_mode_driver <dir>
//       reads what glue_driver reads (a 2-D problem).  One glue instance with hanging_mode = PFM_HANGING_MODE_GATHER: rebuild(),
//       then two rounds of a residual-only and a full assemble().  Writes per round k = 0, 1 <dir>/hm_k<k>_pde.bin, _tot.bin
//       (the residual-only call), _full.bin (system_pde_residual of the full call), _val<b>.bin (the matrix blocks), and
//       <dir>/hm_info.bin: the mode and the five numbers of pfm_ctx_hanging_info after the last call, as doubles.
#define main glue_driver_main
#include "glue_driver.cpp"
#undef main

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
        A.values.assign(A.colind.size(), -7.0e77); // every value must be overwritten
        const long long ncol = blocked ? (c == 0 ? (long long)n_u : (long long)n_nodes) : (long long)(dim + 1) * n_nodes;
        A.colmap.gid.resize((size_t)ncol);
        for (long long g = 0; g < ncol; ++g)
          A.colmap.gid[(size_t)g] = g;
      }
}

template <int dim>
static int run_gather(const std::string &dir, const std::string &meta_text)
{
  const auto sol = read_bin<double>(dir + "/sol.bin"), old = read_bin<double>(dir + "/old.bin"), oldold = read_bin<double>(dir + "/oldold.bin");
  Problem<dim> P;
  int blocked = 0;
  std::istringstream meta(meta_text);
  int d;
  meta >> d;
  setup_problem<dim>(P, dir, std::move(meta), blocked);
  const int nb1 = blocked ? 2 : 1;
  const size_t n0 = blocked ? sol.size() / (dim + 1) * dim : sol.size();
  auto set_vector = [&](TrilinosWrappers::MPI::BlockVector &v, const std::vector<double> &x) {
    v.block(0).v.assign(x.begin(), x.begin() + n0);
    if (blocked)
      v.block(1).v.assign(x.begin() + n0, x.end());
  };
  auto dump = [&](const TrilinosWrappers::MPI::BlockVector &v, const std::string &path) {
    std::vector<double> x;
    for (int b = 0; b < nb1; ++b)
      x.insert(x.end(), v.block(b).begin(), v.block(b).end());
    write_bin(path, x.data(), x.size());
  };
  set_vector(P.solution, sol);
  set_vector(P.old_solution, old);
  set_vector(P.old_old_solution, oldold);
  const std::vector<double> zeros(sol.size(), 0.0);
  set_vector(P.system_pde_residual, zeros);
  set_vector(P.system_total_residual, zeros);
  pfm_glue_detail::PfmGlue<dim> glue;
  glue.hanging_mode = PFM_HANGING_MODE_GATHER;
  glue.rebuild(P);
  for (int k = 0; k < 2; ++k)
    {
      const std::string tag = dir + "/hm_k" + std::to_string(k);
      glue.assemble(P, /*residual_only=*/true);
      dump(P.system_pde_residual, tag + "_pde.bin");
      dump(P.system_total_residual, tag + "_tot.bin");
      glue.assemble(P, /*residual_only=*/false);
      dump(P.system_pde_residual, tag + "_full.bin");
      for (int r = 0; r < nb1; ++r)
        for (int c = 0; c < nb1; ++c)
          {
            const Epetra_CrsMatrix &A = P.system_pde_matrix.block(r, c).trilinos_matrix();
            write_bin(tag + "_val" + std::to_string(2 * r + c) + ".bin", A.values.data(), A.values.size());
          }
    }
  int mode = -1;
  int64_t out[5] = {-1, -1, -1, -1, -1};
  if (pfm_ctx_hanging_info(glue.ctx, &mode, out) != PFM_OK)
    throw std::runtime_error("pfm_ctx_hanging_info");
  const double info[6] = {(double)mode, (double)out[0], (double)out[1], (double)out[2], (double)out[3], (double)out[4]};
  write_bin(dir + "/hm_info.bin", info, (size_t)6);
  std::printf("glue_hanging_mode_driver: OK\n");
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 2)
    {
      std::fprintf(stderr, "usage: glue_hanging_mode_driver <dir>\n");
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
      if (dim != 2)
        throw std::runtime_error("this driver runs the 2-D meshes");
      return run_gather<2>(dir, ss.str());
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "glue_hanging_mode_driver: FAILED: %s\n", e.what());
      return 1;
    }
}

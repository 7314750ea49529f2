// tests/cpp/glue_as_driver.cpp — TEST SCAFFOLDING like glue_ls_driver.cpp (whose problem set-up it repeats on glue_driver.cpp's
// Problem): PfmGlue::active_set_update() on one rank (tests/test_gpu_glue_active_set.py).
//
//   glue_as_driver <dir> <c>
//       reads what glue_driver reads.  assemble(residual_only) with the residuals left on the device, reset_cycle_counter(),
//       then two updates with the constant <c>, the second from what the first left; per update k it writes
//       <dir>/as_k<k>_sol.bin (P.solution), _flags.bin (glue.flags by vertex rank), _cyc.bin (the cycle counter by vertex rank,
//       int32) and _counts.bin (active, cycling, changed as int64)
#define main glue_driver_main
#include "glue_driver.cpp"
#undef main

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

// the owned part of a block vector in the glue's order: block 0, then block 1
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
static int run_as(const std::string &dir, const std::string &meta_text, double c_const)
{
  const auto sol = read_bin<double>(dir + "/sol.bin");
  const auto old = read_bin<double>(dir + "/old.bin"), oldold = read_bin<double>(dir + "/oldold.bin");
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
  const std::vector<double> marker(sol.size(), -7.0e77);
  set_vector(P.system_total_residual, marker, n0);
  pfm_glue_detail::PfmGlue<dim> glue;
  glue.residual_to_host = false;
  glue.active_set_on_device = true;
  glue.rebuild(P);
  glue.assemble(P, /*residual_only=*/true);
  glue.reset_cycle_counter();
  const size_t nn = (size_t)glue.n_nodes;
  const gidx n_u = (gidx)dim * (gidx)nn;
  for (int k = 0; k < 2; ++k)
    {
      const std::array<int64_t, 3> counts = glue.active_set_update(P, c_const);
      if (get_vector(P.system_total_residual) != marker)
        throw std::runtime_error("active_set_update() moved system_total_residual");
      std::vector<int32_t> cyc_node(nn, 0), cyc(nn, 0);
      if (hipMemcpy(cyc_node.data(), glue.d_cycle, sizeof(int32_t) * nn, hipMemcpyDeviceToHost) != hipSuccess)
        throw std::runtime_error("D2H of the cycle counter");
      std::vector<uint8_t> fl(nn, 0);
      for (size_t n = 0; n < nn; ++n)
        {
          const gidx gphi = glue.phi_dof_of_node[n];
          const size_t rank = blocked ? (size_t)(gphi - n_u) : (size_t)((gphi - dim) / (dim + 1));
          fl[rank] = glue.flags[n];
          cyc[rank] = cyc_node[n];
        }
      const std::string tag = dir + "/as_k" + std::to_string(k);
      const std::vector<double> s = get_vector(P.solution);
      write_bin(tag + "_sol.bin", s.data(), s.size());
      write_bin(tag + "_flags.bin", fl.data(), fl.size());
      write_bin(tag + "_cyc.bin", cyc.data(), cyc.size());
      write_bin(tag + "_counts.bin", counts.data(), counts.size());
    }
  std::printf("glue_as_driver: OK\n");
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 3)
    {
      std::fprintf(stderr, "usage: glue_as_driver <dir> <c>\n");
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
      const double c_const = std::strtod(argv[2], nullptr);
      return dim == 2 ? run_as<2>(dir, ss.str(), c_const) : run_as<3>(dir, ss.str(), c_const);
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "glue_as_driver: FAILED: %s\n", e.what());
      return 1;
    }
}

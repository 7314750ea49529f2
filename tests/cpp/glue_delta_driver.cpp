// tests/cpp/glue_delta_driver.cpp — TEST SCAFFOLDING like glue_driver.cpp (whose Problem and file helpers it reuses): two
// Newton iterations of one time step through PfmGlue::assemble(), once with delta_values = true and once, on a second
// glue instance with its own "Trilinos" objects, with the switch off (tests/test_gpu_glue_delta.py).
//
//   glue_delta_driver <dir>   reads what glue_driver reads plus <dir>/sol2.bin (the solution of the second iteration);
//                             writes <dir>/out_val<b>.bin (delta) and <dir>/out_plain_val<b>.bin (switch off) after the
//                             second assemble(), <dir>/out_first_val<b>.bin (delta) after the first, and
//                             <dir>/out_delta_stats.bin (the ten counters of both delta calls)
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
  const std::vector<double> zeros((size_t)(dim + 1) * n_nodes, 0.0);
  for (auto *v : {&P.solution, &P.old_solution, &P.old_old_solution, &P.system_pde_residual, &P.system_total_residual})
    {
      if (blocked)
        {
          v->block(0).v.assign((size_t)n_u, 0.0);
          v->block(1).v.assign((size_t)n_nodes, 0.0);
        }
      else
        v->block(0).v = zeros;
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
static void set_vector(TrilinosWrappers::MPI::BlockVector &v, const std::vector<double> &x, bool blocked)
{
  if (blocked)
    {
      const size_t n_u = v.block(0).v.size();
      v.block(0).v.assign(x.begin(), x.begin() + n_u);
      v.block(1).v.assign(x.begin() + n_u, x.end());
    }
  else
    v.block(0).v = x;
}

template <int dim>
static int run_delta(const std::string &dir, const std::string &meta_text)
{
  const auto sol = read_bin<double>(dir + "/sol.bin"), sol2 = read_bin<double>(dir + "/sol2.bin");
  const auto old = read_bin<double>(dir + "/old.bin"), oldold = read_bin<double>(dir + "/oldold.bin");
  std::vector<int64_t> stats;
  for (int with_delta = 1; with_delta >= 0; --with_delta)
    {
      Problem<dim> P;
      int blocked = 0;
      std::istringstream meta(meta_text);
      int d;
      meta >> d;
      setup_problem<dim>(P, dir, std::move(meta), blocked);
      set_vector<dim>(P.solution, sol, blocked);
      set_vector<dim>(P.old_solution, old, blocked);
      set_vector<dim>(P.old_old_solution, oldold, blocked);
      const int nb1 = blocked ? 2 : 1;
      auto dump = [&](const std::string &prefix) {
        for (int r = 0; r < nb1; ++r)
          for (int c = 0; c < nb1; ++c)
            {
              const Epetra_CrsMatrix &A = P.system_pde_matrix.block(r, c).trilinos_matrix();
              write_bin(dir + "/" + prefix + std::to_string(2 * r + c) + ".bin", A.values.data(), A.values.size());
            }
      };
      pfm_glue_detail::PfmGlue<dim> glue;
      glue.pin_host_matrix = true;
      glue.delta_values = with_delta != 0;
      glue.rebuild(P);
      glue.assemble(P, /*residual_only=*/false);
      if (with_delta)
        {
          dump("out_first_val");
          stats.insert(stats.end(), glue.delta_stats, glue.delta_stats + 10);
        }
      set_vector<dim>(P.solution, sol2, blocked); // the next Newton iteration of the same time step
      glue.assemble(P, /*residual_only=*/false, /*only_solution_changed=*/true);
      dump(with_delta ? "out_val" : "out_plain_val");
      if (with_delta)
        stats.insert(stats.end(), glue.delta_stats, glue.delta_stats + 10);
      glue.before_setup_system(); // drops the context, its page locks and the delta state
    }
  write_bin(dir + "/out_delta_stats.bin", stats.data(), stats.size());
  std::printf("glue_delta_driver: OK (second call moved %lld of %lld bytes)\n", (long long)stats[10], (long long)stats[11]);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 2)
    {
      std::fprintf(stderr, "usage: glue_delta_driver <dir>\n");
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
      return dim == 2 ? run_delta<2>(dir, ss.str()) : run_delta<3>(dir, ss.str());
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "glue_delta_driver: FAILED: %s\n", e.what());
      return 1;
    }
}

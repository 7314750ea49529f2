// tests/cpp/glue_ls_driver.cpp — TEST SCAFFOLDING like glue_driver.cpp (whose Problem and file helpers it reuses):
// PfmGlue::line_search() on one rank in both forms, line_search_stepwise false (one pfm_line_search_device call) and true
// (the host loop of a rank with ghost peers), each on a glue instance with its own "Trilinos" objects
// (tests/test_gpu_glue_line_search.py).
//
//   glue_ls_driver <dir> <use_linfty> <restore_subtract> <reference>
//       reads what glue_driver reads plus <dir>/upd.bin (newton_update).  Per form f = 0 (device) / 1 (stepwise) it runs three
//       searches of at most 4 steps with damping 0.6 from the same state -- reference +inf, 0 and <reference> -- and writes
//       <dir>/ls_f<f>_k<k>_sol.bin, _tot.bin (P.solution, P.system_total_residual) and _res.bin (steps, accepted, norms[3],
//       linf_block[2] as doubles)
#define main glue_driver_main
#include "glue_driver.cpp"
#undef main

#include <limits>

// FracturePhaseFieldProblem<dim>::newton_update next to the members of glue_driver.cpp's Problem
template <int dim>
struct LsProblem : Problem<dim>
{
  TrilinosWrappers::MPI::BlockVector newton_update;
};

template <int dim>
static void setup_problem(LsProblem<dim> &P, const std::string &dir, std::istringstream meta /* behind dim */, int &blocked_out)
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
static int run_ls(const std::string &dir, const std::string &meta_text, bool use_linfty, bool restore_subtract, double reference)
{
  const auto sol = read_bin<double>(dir + "/sol.bin"), upd = read_bin<double>(dir + "/upd.bin");
  const auto old = read_bin<double>(dir + "/old.bin"), oldold = read_bin<double>(dir + "/oldold.bin");
  const double references[3] = {std::numeric_limits<double>::infinity(), 0.0, reference};
  for (int stepwise = 0; stepwise < 2; ++stepwise)
    {
      LsProblem<dim> P;
      int blocked = 0;
      std::istringstream meta(meta_text);
      int d;
      meta >> d;
      setup_problem<dim>(P, dir, std::move(meta), blocked);
      const size_t n0 = blocked ? sol.size() / (dim + 1) * dim : sol.size();
      set_vector(P.old_solution, old, n0);
      set_vector(P.old_old_solution, oldold, n0);
      const std::vector<double> marker(sol.size(), -7.0e77);
      pfm_glue_detail::PfmGlue<dim> glue;
      glue.line_search_stepwise = stepwise != 0;
      glue.residual_to_host = false; // the residuals stay on the device: line_search() must refresh system_total_residual itself
      glue.rebuild(P);
      for (int k = 0; k < 3; ++k)
        {
          set_vector(P.solution, sol, n0);
          set_vector(P.newton_update, upd, n0);
          set_vector(P.system_total_residual, marker, n0);
          glue.assemble(P, /*residual_only=*/true, /*only_solution_changed=*/k > 0);
          if (get_vector(P.system_total_residual) != marker)
            throw std::runtime_error("assemble() with residual_to_host == false wrote system_total_residual");
          const pfm_line_search_result r = glue.line_search(P, references[k], 4, 0.6, use_linfty, restore_subtract);
          const std::string tag = dir + "/ls_f" + std::to_string(stepwise) + "_k" + std::to_string(k);
          const std::vector<double> s = get_vector(P.solution), t = get_vector(P.system_total_residual);
          write_bin(tag + "_sol.bin", s.data(), s.size());
          write_bin(tag + "_tot.bin", t.data(), t.size());
          const double res[7] = {(double)r.steps, (double)r.accepted, r.norms[0], r.norms[1], r.norms[2], r.linf_block[0], r.linf_block[1]};
          write_bin(tag + "_res.bin", res, (size_t)7);
          if (get_vector(P.newton_update) != upd)
            throw std::runtime_error("line_search() wrote P.newton_update");
        }
      {
        // active_set_on_device: the total residual stays on the device until the host asks for it
        glue.active_set_on_device = true;
        set_vector(P.solution, sol, n0);
        set_vector(P.system_total_residual, marker, n0);
        glue.assemble(P, /*residual_only=*/true, /*only_solution_changed=*/true);
        (void)glue.line_search(P, 0.0, 2, 0.6, use_linfty, restore_subtract);
        if (get_vector(P.system_total_residual) != marker)
          throw std::runtime_error("line_search() with active_set_on_device moved system_total_residual");
        glue.fetch_total_residual(P);
        if (get_vector(P.system_total_residual) == marker)
          throw std::runtime_error("fetch_total_residual() left system_total_residual as it was");
      }
    }
  std::printf("glue_ls_driver: OK\n");
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 5)
    {
      std::fprintf(stderr, "usage: glue_ls_driver <dir> <use_linfty> <restore_subtract> <reference>\n");
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
      const bool linfty = std::atoi(argv[2]) != 0, subtract = std::atoi(argv[3]) != 0;
      const double reference = std::strtod(argv[4], nullptr);
      return dim == 2 ? run_ls<2>(dir, ss.str(), linfty, subtract, reference) : run_ls<3>(dir, ss.str(), linfty, subtract, reference);
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "glue_ls_driver: FAILED: %s\n", e.what());
      return 1;
    }
}

// mesh_plan_main.cpp -- the mesh analysis of the context build (cracks_amd/csrc/pfm_mesh_plan.cpp, pfm_host_pool.cpp) as a
// stand-alone host program: reads one mesh from a binary file, runs every function of the plan file on it the way
// pfm_ctx_create does, and writes every table they return to a second file as named arrays.  tests/test_mesh_plan_host.py
// builds it with AddressSanitizer and UBSan, runs it at two thread counts and checks the tables in numpy.
//
//   mesh_plan_main <mesh file> <result file>
//
// mesh file:   int64[10] = dim, n_nodes, n_owned, n_cells, n_hanging, box_cells[3], parent entries, material (0/1); then
//              cells int32[n_cells * 2^dim], coords f64[n_nodes * dim], hn_nodes int32, hn_ptr int64[n_hanging + 1],
//              hn_parents int32, and with material: lambda f64[n_cells], mu f64[n_cells]
// result file: records of  uint32 name length, name, one byte element type (B u8, b i8, i i32, q i64, d f64),
//              int64 count, the elements
#include "pfm_mesh_plan.h"
#include "pfm_host_pool.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pfm;

namespace
{
  FILE *g_out = nullptr;
  void put_raw(const std::string &name, char type, const void *p, size_t count, size_t width)
  {
    const uint32_t nl = (uint32_t)name.size();
    const int64_t cnt = (int64_t)count;
    fwrite(&nl, sizeof nl, 1, g_out);
    fwrite(name.data(), 1, nl, g_out);
    fwrite(&type, 1, 1, g_out);
    fwrite(&cnt, sizeof cnt, 1, g_out);
    if (count)
      fwrite(p, width, count, g_out);
  }
  void put(const std::string &n, const uint8_t *p, size_t c) { put_raw(n, 'B', p, c, 1); }
  void put(const std::string &n, const int8_t *p, size_t c) { put_raw(n, 'b', p, c, 1); }
  void put(const std::string &n, const int32_t *p, size_t c) { put_raw(n, 'i', p, c, 4); }
  void put(const std::string &n, const uint32_t *p, size_t c) { put_raw(n, 'i', p, c, 4); }
  void put(const std::string &n, const int64_t *p, size_t c) { put_raw(n, 'q', p, c, 8); }
  void put(const std::string &n, const long long *p, size_t c) { put_raw(n, 'q', p, c, 8); }
  void put(const std::string &n, const double *p, size_t c) { put_raw(n, 'd', p, c, 8); }
  template <class V>
  void put(const std::string &n, const V &v)
  {
    put(n, v.data(), v.size());
  }
  void put1(const std::string &n, int64_t x) { put(n, &x, 1); }

  template <class T>
  std::vector<T> take(FILE *f, size_t n)
  {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n)
      {
        fprintf(stderr, "mesh_plan_main: short mesh file\n");
        exit(2);
      }
    return v;
  }

  void put_colours(const std::string &pre, const Colours &c)
  {
    put(pre + "_ptr", c.ptr);
    put(pre + "_order", c.order.data(), c.ptr.empty() ? 0 : (size_t)c.ptr.back()); // (order holds one entry when no cell is listed)
    put1(pre + "_overflow", c.overflow);
  }
} // namespace

int main(int argc, char **argv)
{
  if (argc != 3)
    return fprintf(stderr, "usage: mesh_plan_main <mesh file> <result file>\n"), 2;
  FILE *in = fopen(argv[1], "rb");
  g_out = fopen(argv[2], "wb");
  if (!in || !g_out)
    return fprintf(stderr, "mesh_plan_main: cannot open the files\n"), 2;
  const std::vector<int64_t> hd = take<int64_t>(in, 10);
  const int dim = (int)hd[0], nv = 1 << dim;
  const int32_t N = (int32_t)hd[1], NO = (int32_t)hd[2], NH = (int32_t)hd[4];
  const int64_t NC = hd[3];
  const std::vector<int32_t> cells = take<int32_t>(in, (size_t)NC * nv);
  const std::vector<double> coords = take<double>(in, (size_t)N * dim);
  const std::vector<int32_t> hn_nodes = take<int32_t>(in, (size_t)NH);
  const std::vector<int64_t> hn_ptr = take<int64_t>(in, (size_t)NH + 1);
  const std::vector<int32_t> hn_parents = take<int32_t>(in, (size_t)hd[8]);
  const std::vector<double> lam = take<double>(in, hd[9] ? (size_t)NC : 0), mu = take<double>(in, hd[9] ? (size_t)NC : 0);
  fclose(in);

  pfm_mesh_desc m;
  memset(&m, 0, sizeof m);
  m.dim = dim;
  m.n_nodes = N;
  m.n_owned_nodes = NO;
  m.n_cells = NC;
  m.cell_nodes = cells.data();
  m.coords = coords.data();
  m.cell_lambda = hd[9] ? lam.data() : nullptr;
  m.cell_mu = hd[9] ? mu.data() : nullptr;
  m.n_hanging = NH;
  m.hn_nodes = hn_nodes.data();
  m.hn_ptr = hn_ptr.data();
  m.hn_parents = hn_parents.data();
  for (int d = 0; d < 3; ++d)
    m.box_cells[d] = (int32_t)hd[5 + d];

  // ---- hanging table
  std::vector<int32_t> hn_index;
  const char *bad = hanging_index(&m, hn_index);
  const std::string err = bad ? bad : "";
  put("hn_error", reinterpret_cast<const uint8_t *>(err.data()), err.size());
  if (bad)
    return fclose(g_out), 0;
  put("hn_index", hn_index);
  const int32_t *hn_idx = hn_index.empty() ? nullptr : hn_index.data();

  // ---- lattice
  LatticeHost lat;
  const bool lattice_ok = detect_lattice(&m, lat);
  put1("lattice_ok", lattice_ok);
  if (lattice_ok)
    {
      const int32_t dims[6] = {lat.NX, lat.NY, lat.NZ, lat.nc[0], lat.nc[1], lat.nc[2]};
      put("lat_dims", dims, 6);
      put("lat_h", lat.h, 3);
      put("local_of_box", lat.local_of_box);
      put("box_of_local", lat.box_of_local);
      std::vector<int32_t> deg((size_t)NO), rows;
      std::vector<uint32_t> masks((size_t)NO);
      for (int32_t n = 0; n < NO; ++n)
        {
          int32_t q[27];
          deg[n] = lattice_row(lat, dim, n, q, masks[n]);
          rows.insert(rows.end(), q, q + deg[n]);
        }
      put("lat_row_deg", deg);
      put("lat_row_mask", masks);
      put("lat_rows", rows);
      Colours par;
      lattice_colours(&m, lat, par);
      put_colours("latcol", par);
    }

  // ---- colour classes and ring of the general family: the caller's cell table, and its structure-of-arrays copy
  const CellView aos{cells.data(), nv, 1};
  std::vector<int32_t> soa_table((size_t)NC * nv);
  for (int64_t k = 0; k < NC; ++k)
    for (int a = 0; a < nv; ++a)
      soa_table[(size_t)a * NC + k] = cells[(size_t)k * nv + a];
  const CellView soa{soa_table.data(), 1, NC};
  bool coloured = dim == 3 && hn_idx; // (the condition of pfm_ctx_create under PFM_HANGING_COLOURED)
  for (int32_t k = 0; k < NH && coloured; ++k)
    coloured = hn_ptr[k + 1] - hn_ptr[k] <= 4;
  put1("hanging_coloured", coloured);
  for (int mode = 0; mode < (coloured ? 2 : 1); ++mode)
    {
      const std::string pre = mode ? "colh" : "col";
      const int64_t *hp = mode ? hn_ptr.data() : nullptr;
      const int32_t *hpar = mode ? hn_parents.data() : nullptr;
      Colours a, b;
      greedy_colours(NC, nv, N, aos, hn_idx, nullptr, nullptr, a, hp, hpar);
      greedy_colours(NC, nv, N, soa, hn_idx, nullptr, nullptr, b, hp, hpar);
      put_colours(pre, a);
      put1(pre + "_soa_same", a.ptr == b.ptr && a.overflow == b.overflow &&
                                std::equal(a.order.begin(), a.order.begin() + a.ptr.back(), b.order.begin()));
      std::vector<uint8_t> ring, ring_b;
      const bool any = ring_cells(NC, nv, N, aos, hn_idx, hn_ptr.data(), hn_parents.data(), ring, mode != 0);
      const bool any_b = ring_cells(NC, nv, N, soa, hn_idx, hn_ptr.data(), hn_parents.data(), ring_b, mode != 0);
      put1(pre + "_ring_any", any);
      put(pre + "_ring", ring);
      put1(pre + "_ring_soa_same", any == any_b && ring == ring_b);
    }
  {
    const std::atomic<bool> cancel{true};
    Colours c;
    greedy_colours(NC, nv, N, aos, hn_idx, nullptr, &cancel, c);
    put1("cancelled", c.cancelled && c.ptr.empty());
  }

  // ---- cells at hanging vertices
  if (hn_idx)
    {
      std::vector<int32_t> hcells;
      raw_vector<int32_t> hcell;
      put1("hcells_ok", hanging_cells(&m, hn_idx, dim == 3 ? 4 : 2, hcells, hcell));
      put("hcells", hcells);
      put("hcell", hcell);
    }

  // ---- cartesian overlay: the plan, then the reduced colour lists of finish_patches2d / 3d
  std::vector<uint8_t> regular, hang;
  if (dim == 2)
    {
      PatchPlan pl = plan_patches2d(&m, hn_index);
      put("regular", pl.regular);
      put("hang", pl.hang);
      put("blk_cells", pl.blk_cells);
      put("blk_nodes", pl.blk_nodes);
      put("rows_general", pl.rows_general);
      put1("n_regular", pl.n_regular);
      put1("n_blocks", pl.n_blocks);
      if (pl.n_blocks)
        regular = pl.regular, hang = pl.hang;
    }
  else
    {
      PatchPlan3 pl = plan_patches3d(&m, hn_index);
      put("regular", pl.regular);
      put("hang", pl.hang);
      put("rows_general", pl.rows_general);
      put1("n_regular", pl.n_regular);
      put1("n_levels", (int64_t)pl.levels.size());
      for (size_t l = 0; l < pl.levels.size(); ++l)
        {
          const Level3 &lv = pl.levels[l];
          const std::string pre = "lv" + std::to_string(l);
          put(pre + "_h", lv.h, 3);
          put(pre + "_lo", lv.lo, 3);
          put(pre + "_dims", lv.dims, 3);
          put(pre + "_node_at", lv.node_at);
          put(pre + "_row_at", lv.row_at);
          put(pre + "_lam", lv.lam);
          put(pre + "_mu", lv.mu);
          put1(pre + "_n_rows", lv.n_rows);
        }
      if (!pl.levels.empty())
        regular = pl.regular, hang = pl.hang;
    }
  if (!regular.empty())
    {
      std::vector<uint8_t> need((size_t)NC, 0);
      for (int64_t k = 0; k < NC; ++k)
        for (int a = 0; a < nv; ++a)
          {
            const int32_t n = cells[(size_t)k * nv + a];
            if (hang[n] || (n < NO && !regular[n]))
              need[k] = 1;
          }
      put("need", need);
      for (int mode = 0; mode < (coloured ? 2 : 1); ++mode)
        {
          Colours red;
          greedy_colours(NC, nv, N, aos, hn_idx, need.data(), nullptr, red, mode ? hn_ptr.data() : nullptr, mode ? hn_parents.data() : nullptr);
          put_colours(mode ? "redh" : "red", red);
        }
    }
  // ---- the scan of the pool header (pfm_ctx_build.cpp: row pointers of a lattice), against a serial one; not part of the result file
  {
    std::vector<long long> a(200000), b(a.size());
    for (size_t i = 0; i < a.size(); ++i)
      a[i] = b[i] = (long long)((i * 2654435761u) >> 27 & 31);
    inclusive_scan_parallel(a.data(), (int64_t)a.size());
    for (size_t i = 1; i < b.size(); ++i)
      b[i] += b[i - 1];
    if (a != b)
      return fprintf(stderr, "mesh_plan_main: inclusive_scan_parallel differs from the serial scan\n"), 1;
  }
  if (fclose(g_out) != 0)
    return fprintf(stderr, "mesh_plan_main: write failed\n"), 2;
  printf("mesh_plan: OK threads=%d\n", host_threads());
  return 0;
}

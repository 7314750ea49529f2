// The list builder of the ordered gather (pfm::hang_gather_lists, cracks_amd/csrc/pfm_mesh_plan.cpp) on hand-made records, as a
// stand-alone host program (tests/test_hanging_gather_host.py builds it with -fsanitize=address,undefined).  Checked for
// quads (nv = 4, KCMP = 7) and hexes (nv = 8, KCMP = 13): rows ascending; the entries of a row ascending by (cell, index);
// every (cell, owned resolved node) and (cell, owned hanging vertex) listed exactly once, under the row of that node; ghost
// nodes never listed; offsets = prefix sum of R * R * KCMP; a record with R = 0xff makes the builder refuse.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "pfm_mesh_plan.h"

namespace
{
  int failures = 0;
#define CHECK(cond)                                                                                                          \
  do                                                                                                                         \
    {                                                                                                                        \
      if (!(cond))                                                                                                           \
        {                                                                                                                    \
          ++failures;                                                                                                        \
          std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);                                                         \
        }                                                                                                                    \
    }                                                                                                                        \
  while (0)

  struct Rec
  {
    std::vector<int32_t> nodes; // resolved nodes, in record order
    int32_t hv[8];              // hanging vertices' nodes, -1: does not hang
    int R;                      // what the record says (0xff: more than 16)
  };

  std::vector<uint8_t> pack(const std::vector<Rec> &recs)
  {
    std::vector<uint8_t> out(recs.size() * (size_t)pfm::PFM_CRES_BYTES, 0xff);
    for (size_t hc = 0; hc < recs.size(); ++hc)
      {
        uint8_t *r = out.data() + hc * (size_t)pfm::PFM_CRES_BYTES;
        int32_t node[16];
        for (int i = 0; i < 16; ++i)
          node[i] = i < (int)recs[hc].nodes.size() ? recs[hc].nodes[(size_t)i] : -1;
        std::memcpy(r, node, sizeof node);
        r[pfm::PFM_CRES_R] = (uint8_t)recs[hc].R;
        std::memcpy(r + pfm::PFM_CRES_HV, recs[hc].hv, sizeof recs[hc].hv);
        const int32_t cell = 100 + (int32_t)hc;
        std::memcpy(r + pfm::PFM_CRES_CELL, &cell, sizeof cell);
      }
    return out;
  }

  void run(int nv, int kcmp)
  {
    const int32_t NO = 10; // nodes 10.. are ghosts
    std::vector<Rec> recs = {
      {{3, 1, 7, 12, 2}, {-1, 8, -1, -1, -1, -1, -1, -1}, 5},
      {{1, 3, 9, 11}, {13, -1, 4, -1, -1, -1, -1, -1}, 4},
      {{0, 1, 2, 3, 7, 9}, {8, -1, -1, 4, -1, -1, 5, -1}, 6}, // (hv[6]: a hex's seventh vertex; not a quad's)
      {{9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 10, 11, 12, 13, 14, 15}, {-1, -1, -1, -1, -1, -1, -1, -1}, 16},
    };
    const std::vector<uint8_t> bytes = pack(recs);
    pfm::HangGatherLists L;
    CHECK(pfm::hang_gather_lists(bytes.data(), (int64_t)recs.size(), nv, kcmp, NO, L));
    // offsets
    CHECK(L.off.size() == recs.size() + 1 && L.off[0] == 0);
    long long sum = 0;
    for (size_t hc = 0; hc < recs.size() && hc + 1 < L.off.size(); ++hc)
      {
        CHECK(L.off[hc] == sum);
        sum += (long long)recs[hc].R * recs[hc].R * kcmp;
      }
    CHECK(L.off.back() == sum);
    // what must be listed: (row node) -> set of (cell, index)
    std::map<int32_t, std::set<std::pair<int, int>>> want;
    for (size_t hc = 0; hc < recs.size(); ++hc)
      {
        for (int i = 0; i < recs[hc].R; ++i)
          if (recs[hc].nodes[(size_t)i] < NO)
            want[recs[hc].nodes[(size_t)i]].insert({(int)hc, i});
        for (int a = 0; a < nv; ++a)
          if (recs[hc].hv[a] >= 0 && recs[hc].hv[a] < NO)
            want[recs[hc].hv[a]].insert({(int)hc, 16 + a});
      }
    CHECK(L.rows.size() == want.size() && L.ptr.size() == L.rows.size() + 1 && L.ptr[0] == 0);
    CHECK((size_t)L.ptr.back() == L.list.size());
    size_t r = 0;
    for (const auto &kv : want)
      {
        if (r >= L.rows.size())
          break;
        CHECK(L.rows[r] == kv.first);                // rows ascending (std::map iterates ascending), none missing, none extra
        CHECK(L.rows[r] >= 0 && L.rows[r] < NO);     // ghosts never listed
        CHECK(r == 0 || L.rows[r - 1] < L.rows[r]);
        std::set<std::pair<int, int>> got;
        long long prev = -1;
        for (long long e = L.ptr[r]; e < L.ptr[r + 1]; ++e)
          {
            const pfm::HgEntry &en = L.list[(size_t)e];
            CHECK((long long)en.code > prev);        // ascending by (cell, index): code = 32 cell + index, and no entry twice
            prev = en.code;
            const int hc = en.code >> 5, idx = en.code & 31;
            CHECK(hc >= 0 && hc < (int)recs.size());
            if (hc < 0 || hc >= (int)recs.size())
              continue;
            CHECK(en.R == recs[(size_t)hc].R);
            if (idx < 16)
              {
                CHECK(idx < en.R && recs[(size_t)hc].nodes[(size_t)idx] == kv.first);
                CHECK(en.koff == L.off[(size_t)hc] + (long long)idx * en.R * kcmp);
              }
            else
              CHECK(idx - 16 < nv && recs[(size_t)hc].hv[idx - 16] == kv.first);
            got.insert({hc, idx});
          }
        CHECK(got == kv.second);
        ++r;
      }
    // nv decides how many vertex slots are read: node 5 hangs at the seventh vertex of cell 2
    bool has5 = false;
    for (const pfm::HgEntry &en : L.list)
      has5 = has5 || en.code == 2 * 32 + 16 + 6;
    CHECK(has5 == (nv == 8));
    // more than 16 resolved nodes somewhere: refused, nothing filled
    recs[1].R = 0xff;
    const std::vector<uint8_t> bad = pack(recs);
    pfm::HangGatherLists B;
    B.rows.push_back(7);
    CHECK(!pfm::hang_gather_lists(bad.data(), (int64_t)recs.size(), nv, kcmp, NO, B));
    CHECK(B.rows.empty() && B.ptr.empty() && B.list.empty() && B.off.empty());
    // no records at all
    pfm::HangGatherLists E;
    CHECK(pfm::hang_gather_lists(bad.data(), 0, nv, kcmp, NO, E));
    CHECK(E.rows.empty() && E.list.empty() && E.ptr.size() == 1 && E.off.size() == 1 && E.off[0] == 0);
    std::printf("nv %d kcmp %d: %zu rows, %zu entries, %lld scratch doubles\n", nv, kcmp, L.rows.size(), L.list.size(), L.off.back());
  }
} // namespace

int main()
{
  run(4, 7);
  run(8, 13);
  std::printf(failures ? "hang_gather: %d FAILED\n" : "hang_gather: OK\n", failures);
  return failures ? 1 : 0;
}

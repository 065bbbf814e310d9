// Stand-alone check of coral_amd/csrc/gemm_plan.h (host compiler only, no HIP): built and run by test_gemm_plan_cpu.py.
//   1. every row of tests/golden/gemm_plan.json - (descriptor fields, knobs) -> kernel instantiation and launch
//      geometry, recorded from the dispatcher before the rule moved into gemm_plan.h - is reproduced field by field;
//   2. tile_of_block_g over blocks 0 .. tile_grid - 1 visits every tile of the grid exactly once and nothing outside it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../coral_amd/csrc/gemm_plan.h"

static const char* const kColumns[] = {
    "api", "M", "N", "K", "a_layout", "b_layout", "a_kseg", "b_kseg", "batch1", "batch2", "epilogue", "dropout", "a_colsum",
    "c_row_index", "c_split_n", "C8", "c_sumsq", "a_ln", "count", "M1", "N1", "M2", "N2", "M3", "N3",
    "x_persist", "skinny_mb1", "skinny_mb1_rows", "skinny_nt", "skinny_u", "prefer_l", "l_over_x", "l_min", "m_max",
    "force_kernel", "compute_cus", "device_cus",
    "error", "family", "fp8", "lay", "ks", "mb", "nch", "u", "nt", "grid_x", "grid_y", "grid_z", "block", "lds", "vgrid",
    "persistent", "dyn_first", "kind"};
enum { NCOL = sizeof(kColumns) / sizeof(kColumns[0]), NOUT = 18 };

// the table is {"comment": .., "columns": [names], "rows": [[integers], ..]}: enough of JSON for exactly that
static bool read_table(const char* path, std::vector<std::vector<long long>>& rows) {
  std::ifstream f(path);
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string s = ss.str();
  std::string want = "\"columns\": [";
  for (int i = 0; i < NCOL; ++i) want += std::string(i ? ", \"" : "\"") + kColumns[i] + "\"";
  want += "]";
  if (s.find(want) == std::string::npos) {
    fprintf(stderr, "%s: the column list is not the one this program was written for\n", path);
    return false;
  }
  size_t p = s.find("\"rows\"");
  if (p == std::string::npos || (p = s.find('[', p)) == std::string::npos) return false;
  int depth = 0;  // 1 inside "rows", 2 inside a row
  for (; p < s.size(); ++p) {
    const char c = s[p];
    if (c == '[') {
      if (++depth == 2) rows.emplace_back();
    } else if (c == ']') {
      if (--depth == 0) break;
    } else if (depth == 2 && (c == '-' || (c >= '0' && c <= '9'))) {
      char* end = nullptr;
      rows.back().push_back(strtoll(s.c_str() + p, &end, 10));
      p = (size_t)(end - s.c_str()) - 1;
    }
  }
  for (const auto& r : rows)
    if ((int)r.size() != NCOL) {
      fprintf(stderr, "%s: a row has %zu fields, not %d\n", path, r.size(), (int)NCOL);
      return false;
    }
  return !rows.empty();
}

static int check_row(int idx, const std::vector<long long>& r) {
  alignas(16) static char dummy[64];
  int i = 0;
  const int api = (int)r[i++];
  CaGemmDesc d[4];
  memset(d, 0, sizeof d);
  CaGemmDesc& a = d[0];
  a.M = (int)r[i++]; a.N = (int)r[i++]; a.K = (int)r[i++];
  a.a_layout = (int)r[i++]; a.b_layout = (int)r[i++];
  a.a_kseg = (int)r[i++]; a.b_kseg = (int)r[i++];
  a.batch1 = (int)r[i++]; a.batch2 = (int)r[i++];
  a.epilogue = (int)r[i++];
  a.dropout_p = r[i++] ? 0.1f : 0.f;
  a.a_colsum = r[i++] ? (float*)dummy : nullptr;
  a.c_row_index = r[i++] ? (const int32_t*)dummy : nullptr;
  a.c_split_n = (int)r[i++];
  a.C8 = r[i++] ? (void*)dummy : nullptr;
  a.c_sumsq = r[i++] ? (float*)dummy : nullptr;
  a.a_ln_gamma = r[i++] ? (const float*)dummy : nullptr;
  const int count = (int)r[i++];
  for (int j = 1; j < 4; ++j) {
    d[j] = a;
    d[j].M = (int)r[i++];
    d[j].N = (int)r[i++];
  }
  GemmKnobs k;
  k.x_persist = (int)r[i++]; k.skinny_mb1 = (int)r[i++]; k.skinny_mb1_rows = (int)r[i++]; k.skinny_nt = (int)r[i++];
  k.skinny_u = (int)r[i++]; k.prefer_l = (int)r[i++]; k.l_over_x = (int)r[i++]; k.l_min = (int)r[i++]; k.m_max = (int)r[i++];
  k.force_kernel = (int)r[i++]; k.compute_cus = (int)r[i++]; k.device_cus = (unsigned)r[i++];
  const GemmPlan p = api == 0 ? gemm_plan_bf16(a, k) : (api == 1 ? gemm_plan_fp8(a, k) : gemm_plan_group(d, count, k));
  const long long got[NOUT] = {p.error, p.family, p.fp8, p.lay, p.ks, p.mb, p.nch, p.u, p.nt, p.grid_x, p.grid_y, p.grid_z,
                               p.block, (long long)p.lds, p.vgrid, p.persistent, p.dyn_first, p.kind};
  const long long* want = r.data() + (NCOL - NOUT);
  int bad = 0;
  const int ncmp = want[0] != 0 ? 1 : NOUT;  // a rejected descriptor launches nothing: only the error is recorded
  for (int o = 0; o < ncmp; ++o)
    if (got[o] != want[o]) {
      fprintf(stderr, "row %d (api %d, M %d N %d K %d): %s = %lld, the table has %lld\n", idx, api, a.M, a.N, a.K,
              kColumns[NCOL - NOUT + o], got[o], want[o]);
      bad = 1;
    }
  return bad;
}

template <int SBM, int SBN>
static int check_cover(bool bal) {
  int bad = 0;
  std::vector<int> hits;
  for (int ntm = 1; ntm <= 64; ++ntm)
    for (int ntn = 1; ntn <= 64; ++ntn) {
      const int grid = (int)tile_grid<SBM, SBN>(ntm, ntn, bal);
      hits.assign((size_t)ntm * ntn, 0);
      int outside = 0;
      for (int b = 0; b < grid; ++b) {
        int tm = -1, tn = -1;
        if (!tile_of_block_g<SBM, SBN>(b, grid, ntm, ntn, tm, tn, bal)) continue;
        if (tm < 0 || tm >= ntm || tn < 0 || tn >= ntn) ++outside;
        else ++hits[(size_t)tm * ntn + tn];
      }
      int wrong = 0;
      for (int h : hits) wrong += h != 1;
      if (outside || wrong) {
        fprintf(stderr, "tile cover <%d, %d> bal %d, %d x %d tiles, grid %d: %d tiles not hit exactly once, %d outside\n", SBM, SBN,
                (int)bal, ntm, ntn, grid, wrong, outside);
        bad = 1;
      }
    }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s tests/golden/gemm_plan.json\n", argv[0]);
    return 2;
  }
  std::vector<std::vector<long long>> rows;
  if (!read_table(argv[1], rows)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  int bad_rows = 0;
  for (size_t i = 0; i < rows.size(); ++i) bad_rows += check_row((int)i, rows[i]);
  const int bad_cover = check_cover<4, 8>(false) + check_cover<4, 8>(true) + check_cover<8, 8>(false) + check_cover<8, 8>(true);
  printf("gemm_plan: %zu rows, %d differ; tile cover %s\n", rows.size(), bad_rows, bad_cover ? "BROKEN" : "ok");
  return bad_rows || bad_cover ? 1 : 0;
}

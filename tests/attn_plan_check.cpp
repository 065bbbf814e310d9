// Stand-alone check of coral_amd/csrc/attn_plan.h (host compiler only, no HIP): built and run by test_attn_plan_cpu.py.
//   1. every row of tests/golden/attn_plan.json - (descriptor fields, knobs) -> kernel instantiations and launch
//      geometry, recorded from the dispatcher before the rule moved into attn_plan.h - is reproduced field by field;
//   2. attn_tile_of over blocks 0 .. attn_grid - 1 visits every (tile, head, clip) exactly once, also where heads x clips
//      is no multiple of 8, and reports every other block as padding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../coral_amd/csrc/attn_plan.h"

static const char* const kColumns[] = {
    "api", "B", "H", "Tq", "Tk", "hd", "causal", "drop", "klen", "row_off", "key_slot", "O8", "ws",
    "wide", "wpe3", "dq_wpe3", "dkv_wide", "dkv_wpe3", "smallq_2percu", "split", "split_tail", "device_cus",
    "error",
    "kernel0", "hdpv0", "drop0", "wpe0", "dt0", "qp0", "ks0", "grid0", "block0", "lds0",
    "kernel1", "hdpv1", "drop1", "wpe1", "dt1", "qp1", "ks1", "grid1", "block1", "lds1",
    "kernel2", "hdpv2", "drop2", "wpe2", "dt2", "qp2", "ks2", "grid2", "block2", "lds2",
    "nsplit", "ns", "tail_start", "ns_tail", "slab_off"};
enum { NCOL = sizeof(kColumns) / sizeof(kColumns[0]), NSLOT = 10, NOUT = 1 + 3 * NSLOT + 5 };

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

static void put_slot(long long* out, const AttnPlan& p) {
  if (p.kernel == ATTN_NONE) return;  // a launch that does not happen is a row of zeros
  const long long v[NSLOT] = {p.kernel, p.hdpv, p.drop, p.wpe, p.dt, p.qp, p.ks, p.grid, p.block, (long long)p.lds};
  memcpy(out, v, sizeof v);
}

static int check_row(int idx, const std::vector<long long>& r) {
  alignas(256) static char dummy[256];
  int i = 0;
  const int api = (int)r[i++];
  CaAttnDesc d;
  memset(&d, 0, sizeof d);
  d.B = (int)r[i++]; d.H = (int)r[i++]; d.Tq = (int)r[i++]; d.Tk = (int)r[i++]; d.hd = (int)r[i++];
  d.Tqp = (d.Tq + 31) / 32 * 32;
  d.causal = (int)r[i++];
  d.dropout_p = r[i++] ? 0.1f : 0.f;
  d.klen = r[i++] ? (const int32_t*)dummy : nullptr;
  d.row_off = r[i++] ? (const int32_t*)dummy : nullptr;
  d.key_slot = r[i++] ? (const int32_t*)dummy : nullptr;
  if (r[i++]) { d.O8 = dummy; d.o8_scale = (const float*)dummy; }
  const int ws = (int)r[i++];
  if (ws) { d.split_ws = dummy; d.split_ws_bytes = CA_ATTN_SPLIT_WS_BYTES(d.B, d.H) - (ws == 2 ? 1 : 0); }
  d.ldo = (int64_t)d.H * d.hd;
  AttnKnobs k;
  k.wide = (int)r[i++]; k.wpe3 = (int)r[i++]; k.dq_wpe3 = (int)r[i++]; k.dkv_wide = (int)r[i++]; k.dkv_wpe3 = (int)r[i++];
  k.smallq_2percu = (int)r[i++]; k.split = (int)r[i++]; k.split_tail = (int)r[i++]; k.device_cus = (int)r[i++];
  long long got[NOUT] = {0};
  long long* split = got + 1 + 3 * NSLOT;
  split[0] = 1;
  if (api == 2) {
    const AttnBwdPlan bp = attn_plan_bwd(d, k);
    got[0] = bp.error;
    put_slot(got + 1, bp.prep);
    put_slot(got + 1 + NSLOT, bp.dq);
    put_slot(got + 1 + 2 * NSLOT, bp.dkv);
  } else {
    const AttnPlan p = api == 0 ? attn_plan_fwd(d, k) : attn_plan_qproj(d, k);
    got[0] = p.error;
    put_slot(got + 1, p);
    if (p.nsplit > 1) {
      const long long v[5] = {p.nsplit, p.split.ns, p.split.tail_start, p.split.ns_tail, (long long)p.slab_off};
      memcpy(split, v, sizeof v);
    }
  }
  const long long* want = r.data() + (NCOL - NOUT);
  int bad = 0;
  const int ncmp = want[0] != 0 ? 1 : NOUT;  // a rejected descriptor launches nothing: only the error is recorded
  for (int o = 0; o < ncmp; ++o)
    if (got[o] != want[o]) {
      fprintf(stderr, "row %d (api %d, B %d H %d Tq %d Tk %d hd %d): %s = %lld, the table has %lld\n", idx, api, d.B, d.H, d.Tq,
              d.Tk, d.hd, kColumns[NCOL - NOUT + o], got[o], want[o]);
      bad = 1;
    }
  return bad;
}

static int check_cover() {
  int bad = 0;
  std::vector<int> hits;
  for (int ntile = 1; ntile <= 9; ++ntile)
    for (int hb = 1; hb <= 40; ++hb)
      for (int H = 1; H <= hb; ++H) {
        if (hb % H) continue;
        const int B = hb / H, grid = (int)attn_grid(ntile, H, B);
        hits.assign((size_t)ntile * hb, 0);
        int outside = 0, padding = 0;
        for (int blk = 0; blk < grid; ++blk) {
          int tile = -1, h = -1, b = -1;
          if (!attn_tile_of(blk, ntile, H, B, tile, h, b)) {
            ++padding;
            continue;
          }
          if (tile < 0 || tile >= ntile || h < 0 || h >= H || b < 0 || b >= B) ++outside;
          else ++hits[((size_t)b * H + h) * ntile + tile];
        }
        int wrong = 0;
        for (int n : hits) wrong += n != 1;
        if (outside || wrong || padding != grid - ntile * hb) {
          fprintf(stderr, "tile cover, %d tiles x %d heads x %d clips, grid %d: %d not hit exactly once, %d outside, %d padding\n",
                  ntile, H, B, grid, wrong, outside, padding);
          bad = 1;
        }
      }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s tests/golden/attn_plan.json\n", argv[0]);
    return 2;
  }
  std::vector<std::vector<long long>> rows;
  if (!read_table(argv[1], rows)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  int bad_rows = 0;
  for (size_t i = 0; i < rows.size(); ++i) bad_rows += check_row((int)i, rows[i]);
  const int bad_cover = check_cover();
  printf("attn_plan: %zu rows, %d differ; tile cover %s\n", rows.size(), bad_rows, bad_cover ? "BROKEN" : "ok");
  return bad_rows || bad_cover ? 1 : 0;
}

// Host program of tests/test_gemm_plan_host.py: includes ONLY csrc/gemm_plan.h, reads the blocks of tests/golden/gemm_dispatch.json
// (["planner", [[values of input column 0], [values of column 1], ...], [answers]]) and prints, for every case of every block (the
// cartesian product of the value lists, last column fastest), the planner's name and what the planner answers.
#include "gemm_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace smd_plan;

static void answer(const std::string& tag, const std::vector<long>& v) {
  if (tag == "nt") {
    const NtEpiFlags fl = {(int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10]};
    const NtKnobs kn = {(int)v[12], (int)v[13], (int)v[14], (int)v[15], (int)v[16], (int)v[17]};
    const NtPlan p = nt_plan((int)v[0], (int)v[1], (int)v[2], fl, (int)v[11], kn);
    printf("nt %d %d %d %d %d %d %d %d\n", p.kernel, p.BM, p.NS, p.KG, p.grid, p.block, p.pk_epilogue, p.vec_epilogue);
  } else if (tag == "tn128") {
    const TnKnobs kn = {(int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9]};
    const TnSite site = v[3] ? TN_SINGLE : TN_GROUPED;
    const TnSplit sp = tn128_split((int)v[0], (int)v[1], (size_t)v[2], site, kn);
    const TnMode m = tn128_mode(sp.ktiles_per_split, site, kn);
    printf("tn128 %d %d %d %d %d\n", sp.nsplit, sp.ktiles_per_split, m.ns, m.nw, m.pad_bytes);
  } else if (tag == "tn256") {
    const TnSplit sp = tn256_plan((int)v[0], (int)v[1], (int)v[2], (size_t)v[3], (int)v[4]);
    printf("tn256 %d %d\n", sp.nsplit, sp.ktiles_per_split);
  } else {
    const TnSplit sp = tn256_multi_split((int)v[0], (int)v[1]);
    printf("tn256_multi %d %d\n", sp.nsplit, sp.ktiles_per_split);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s gemm_dispatch.json\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::string s;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
  fclose(f);
  size_t pos = 0, nblocks = 0;
  while ((pos = s.find("[\"", pos)) != std::string::npos) {            // a block: ["planner", [[...], [...], ...], [answers]]
    const size_t q = s.find('"', pos + 2);
    const std::string tag = s.substr(pos + 2, q - pos - 2);
    const size_t need = tag == "nt" ? 18 : tag == "tn128" ? 10 : tag == "tn256" ? 5 : tag == "tn256_multi" ? 2 : 0;
    pos = s.find('[', q);                                              // the list of value lists
    if (!need || pos == std::string::npos) { fprintf(stderr, "block %zu: unknown planner '%s'\n", nblocks, tag.c_str()); return 3; }
    std::vector<std::vector<long>> axes;
    for (++pos; pos < s.size() && s[pos] != ']'; ++pos) {
      if (s[pos] != '[') continue;
      axes.emplace_back();
      const size_t end = s.find(']', pos);
      for (const char* p = s.c_str() + pos + 1; p < s.c_str() + end;) {
        char* e;
        const long x = strtol(p, &e, 10);
        if (e == p) ++p; else { axes.back().push_back(x); p = e; }
      }
      if (axes.back().empty()) { fprintf(stderr, "block %zu: empty value list\n", nblocks); return 3; }
      pos = end;
    }
    if (axes.size() != need) { fprintf(stderr, "block %zu (%s): %zu input columns, %zu needed\n", nblocks, tag.c_str(), axes.size(), need); return 3; }
    std::vector<size_t> at(need, 0);
    std::vector<long> v(need);
    for (bool more = true; more;) {
      for (size_t c = 0; c < need; ++c) v[c] = axes[c][at[c]];
      answer(tag, v);
      more = false;
      for (size_t c = need; c-- > 0;) {                                // odometer, last column fastest
        if (++at[c] < axes[c].size()) { more = true; break; }
        at[c] = 0;
      }
    }
    ++nblocks;
  }
  return nblocks ? 0 : 4;
}

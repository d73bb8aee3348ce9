// Length-limited Huffman code lengths by package-merge (include/ttvdm.h, "PNG export", rule 4): the one builder behind
// tt_png_code_lengths, tt_png_plan and tt_jpeg_optimized_table.  Header-only, plain C++17, no HIP include.  What turns lengths into codes
// stays with each format: DEFLATE and JPEG order their bits differently.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "ttvdm.h"
#include "host_common.h"

struct TtHuffItem {
  uint64_t weight;
  bool leaf;
};

// `used` symbols in ascending (count, symbol); lengths is zeroed by the caller.  false: 2^limit < used symbols
inline bool tt_package_merge(const uint32_t* counts, const std::vector<int>& used, int limit, uint8_t* lengths) {
  const size_t u = used.size(), keep = 2 * u - 2;
  std::vector<std::vector<TtHuffItem>> lists((size_t)limit);
  for (int s : used) lists[0].push_back({counts[s], true});
  for (int l = 1; l < limit; ++l) {
    const std::vector<TtHuffItem>& prev = lists[l - 1];
    std::vector<TtHuffItem>& cur = lists[l];
    cur.reserve(keep);
    size_t leaf = 0, pack = 0;
    const size_t packs = prev.size() / 2;
    while (cur.size() < keep && (leaf < u || pack < packs)) {
      const uint64_t pw = pack < packs ? prev[2 * pack].weight + prev[2 * pack + 1].weight : 0;
      if (leaf < u && (pack >= packs || counts[used[leaf]] <= pw)) cur.push_back({counts[used[leaf++]], true});      // <=: a leaf before a package
      else { cur.push_back({pw, false}); ++pack; }
    }
  }
  size_t take = keep;
  if (lists[limit - 1].size() < take) return false;
  for (int l = limit - 1; l >= 0 && take > 0; --l) {
    size_t leaves = 0;
    for (size_t i = 0; i < take; ++i) leaves += lists[l][i].leaf;
    for (size_t i = 0; i < leaves; ++i) ++lengths[used[i]];
    take = 2 * (take - leaves);
  }
  return true;
}

// lengths[0 .. nsym) of codes of at most `limit` bits for the symbols with a count; `who` names the caller in a refusal
inline int tt_code_lengths(const char* who, const uint32_t* counts, int nsym, int limit, uint8_t* lengths) {
  std::vector<int> used;
  for (int s = 0; s < nsym; ++s)
    if (counts[s]) used.push_back(s);
  memset(lengths, 0, (size_t)nsym);
  if (used.empty()) TT_FAIL(TT_EINVAL, "%s: no used symbol among %d", who, nsym);
  if (used.size() == 1) { lengths[used[0]] = 1; return TT_OK; }
  if (((size_t)1 << limit) < used.size()) TT_FAIL(TT_EINVAL, "%s: %d used symbols do not fit codes of at most %d bits", who, (int)used.size(), limit);
  std::stable_sort(used.begin(), used.end(), [&](int a, int b) { return counts[a] < counts[b]; });       // stable: ascending symbol inside a count
  if (!tt_package_merge(counts, used, limit, lengths)) TT_FAIL(TT_EINVAL, "%s: package-merge ran out of items (limit %d)", who, limit);
  return TT_OK;
}

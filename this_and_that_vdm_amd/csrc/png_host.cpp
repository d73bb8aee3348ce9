// libttvdm: the host half of the PNG export -- tt_png_code_lengths (length-limited Huffman code lengths by package-merge),
// tt_png_block_header (the dynamic-block header of one stripe and the stripe's exact size) and tt_png_plan (both for every stripe of a
// call, with the code tables and byte offsets tt_png_emit reads).  include/ttvdm.h states them rule by rule; integers only.
#include "png_host.h"

#include "huffman_host.h"

#include <string.h>
#include <vector>

namespace {

// canonical codes (RFC 1951 3.2.2) with their bits reversed: ready to be ORed in from the least significant bit
void reversed_codes(const uint8_t* lengths, int nsym, uint32_t* codes) {
  int per[16] = {0};
  for (int s = 0; s < nsym; ++s) ++per[lengths[s]];
  per[0] = 0;
  uint32_t next[16] = {0}, code = 0;
  for (int b = 1; b <= 15; ++b) { code = (code + (uint32_t)per[b - 1]) << 1; next[b] = code; }
  for (int s = 0; s < nsym; ++s) {
    uint32_t c = lengths[s] ? next[lengths[s]]++ : 0, r = 0;
    for (int b = 0; b < lengths[s]; ++b, c >>= 1) r = (r << 1) | (c & 1u);
    codes[s] = r;
  }
}

struct BitSink {                                   // bits from the least significant bit of each word; at most 16 per put
  uint32_t* words;
  int cap_bits, n = 0;
  bool full = false;
  BitSink(uint32_t* w, int cap_words) : words(w), cap_bits(cap_words * 32) { memset(w, 0, (size_t)cap_words * 4); }
  void put(uint32_t v, int k) {
    if (n + k > cap_bits) { full = true; return; }
    const int word = n >> 5, sh = n & 31;
    words[word] |= v << sh;
    if (sh + k > 32) words[word + 1] |= v >> (32 - sh);
    n += k;
  }
};

struct ClToken { uint8_t sym, extra_bits, extra; };

// rule 5's greedy run coding of the HLIT + 257 literal/length lengths and the one distance length
void run_code(const std::vector<uint8_t>& seq, std::vector<ClToken>& out) {
  for (size_t i = 0; i < seq.size();) {
    const uint8_t v = seq[i];
    size_t run = 1;
    while (i + run < seq.size() && seq[i + run] == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) { const size_t t = run < 138 ? run : 138; out.push_back({18, 7, (uint8_t)(t - 11)}); run -= t; }
      if (run >= 3) { out.push_back({17, 3, (uint8_t)(run - 3)}); run = 0; }
    } else {
      out.push_back({v, 0, 0});
      --run;
      while (run >= 3) { const size_t t = run < 6 ? run : 6; out.push_back({16, 2, (uint8_t)(t - 3)}); run -= t; }
    }
    for (; run > 0; --run) out.push_back({v, 0, 0});
  }
}

const uint8_t CL_ORDER[TT_PNG_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

int block_header(const char* who, const uint32_t* counts, const uint8_t* lengths, uint32_t* header, int32_t cap_words, int64_t* stripe_bits_out) {
  if (cap_words < TT_PNG_HEADER_WORDS) TT_FAIL(TT_EINVAL, "%s: cap too small: %d words, a header takes up to %d (TT_PNG_HEADER_WORDS)", who, cap_words, TT_PNG_HEADER_WORDS);
  uint64_t kraft = 0;
  int last = 256;
  int64_t data_bits = 0;
  for (int s = 0; s < TT_PNG_SYMS; ++s) {
    if (lengths[s] > TT_PNG_LIT_LIMIT) TT_FAIL(TT_EINVAL, "%s: lengths[%d] = %d (at most %d)", who, s, lengths[s], TT_PNG_LIT_LIMIT);
    if ((counts[s] || s == 256) && !lengths[s]) TT_FAIL(TT_EINVAL, "%s: symbol %d is used and has no length", who, s);
    if (lengths[s]) { kraft += 1ull << (TT_PNG_LIT_LIMIT - lengths[s]); if (s > last) last = s; }
    data_bits += (int64_t)counts[s] * (lengths[s] + (s > 256 ? tt_png_length_extra(s) + 1 : 0));      // + 1: the match's distance bit
  }
  if (kraft > (1ull << TT_PNG_LIT_LIMIT)) TT_FAIL(TT_EINVAL, "%s: the lengths' Kraft sum exceeds 1", who);
  const int hlit = last + 1;
  std::vector<uint8_t> seq(lengths, lengths + hlit);
  seq.push_back(1);
  std::vector<ClToken> toks;
  run_code(seq, toks);
  uint32_t cl_counts[TT_PNG_CL_SYMS] = {0}, cl_codes[TT_PNG_CL_SYMS];
  uint8_t cl_len[TT_PNG_CL_SYMS];
  for (const ClToken& t : toks) ++cl_counts[t.sym];
  const int rc = tt_code_lengths(who, cl_counts, TT_PNG_CL_SYMS, TT_PNG_CL_LIMIT, cl_len);
  if (rc != TT_OK) return rc;
  reversed_codes(cl_len, TT_PNG_CL_SYMS, cl_codes);
  int hclen = 4;
  for (int i = 4; i < TT_PNG_CL_SYMS; ++i)
    if (cl_len[CL_ORDER[i]]) hclen = i + 1;
  BitSink sink(header + 1, cap_words - 1);
  sink.put(0, 1);                                   // BFINAL
  sink.put(2, 2);                                   // BTYPE: dynamic codes
  sink.put((uint32_t)(hlit - 257), 5);
  sink.put(0, 5);                                   // HDIST - 1: one distance code
  sink.put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) sink.put(cl_len[CL_ORDER[i]], 3);
  for (const ClToken& t : toks) {
    sink.put(cl_codes[t.sym], cl_len[t.sym]);
    if (t.extra_bits) sink.put(t.extra, t.extra_bits);
  }
  if (sink.full) TT_FAIL(TT_EINVAL, "%s: cap too small: the header does not fit %d words", who, cap_words);
  header[0] = (uint32_t)sink.n;
  *stripe_bits_out = sink.n + data_bits + 3;
  return TT_OK;
}

}  // namespace

extern "C" int64_t tt_png_stream_bytes(int32_t h, int32_t w, int32_t ch) {
  return tt_png_shape_ok(1, h, w, ch) ? (int64_t)h * (1 + (int64_t)w * ch) : 0;
}
extern "C" int64_t tt_png_frame_stride(int32_t h, int32_t w, int32_t ch) { return (tt_png_stream_bytes(h, w, ch) + 15) / 16 * 16; }
extern "C" int64_t tt_png_stripes(int32_t h, int32_t w, int32_t ch) { return (tt_png_stream_bytes(h, w, ch) + TT_PNG_STRIPE - 1) / TT_PNG_STRIPE; }

extern "C" int tt_png_code_lengths(const uint32_t* counts, int32_t nsym, int32_t limit, uint8_t* lengths) {
  if (!counts || !lengths) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: null %s", !counts ? "counts" : "lengths");
  if (nsym < 1 || nsym > TT_PNG_SYMS) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: nsym = %d (1 to %d)", nsym, TT_PNG_SYMS);
  if (limit < 1 || limit > TT_PNG_LIT_LIMIT) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: limit = %d (1 to %d)", limit, TT_PNG_LIT_LIMIT);
  return tt_code_lengths("tt_png_code_lengths", counts, nsym, limit, lengths);
}

extern "C" int tt_png_block_header(const uint32_t* counts, const uint8_t* lengths, uint32_t* header, int32_t cap_words, int64_t* stripe_bits_out) {
  if (!counts || !lengths || !header || !stripe_bits_out)
    TT_FAIL(TT_EINVAL, "tt_png_block_header: null %s", !counts ? "counts" : (!lengths ? "lengths" : (!header ? "header" : "stripe_bits_out")));
  return block_header("tt_png_block_header", counts, lengths, header, cap_words, stripe_bits_out);
}

extern "C" int tt_png_plan(const uint32_t* records, int64_t nstripes, uint32_t* tables, uint32_t* headers, int64_t* total_bytes_out) {
  if (!records || !tables || !headers || !total_bytes_out)
    TT_FAIL(TT_EINVAL, "tt_png_plan: null %s", !records ? "records" : (!tables ? "tables" : (!headers ? "headers" : "total_bytes_out")));
  if (nstripes <= 0) TT_FAIL(TT_EINVAL, "tt_png_plan: nstripes = %lld", (long long)nstripes);
  int64_t offset = 0;
  uint8_t lengths[TT_PNG_SYMS];
  for (int64_t i = 0; i < nstripes; ++i) {
    const uint32_t* counts = records + i * TT_PNG_RECORD_WORDS;
    uint32_t* table = tables + i * TT_PNG_TABLE_WORDS;
    uint64_t tokens = 0;
    for (int s = 0; s < TT_PNG_SYMS; ++s) tokens += counts[s];
    if (counts[256] != 1 || tokens < 2 || tokens > TT_PNG_STRIPE + 1)
      TT_FAIL(TT_EINVAL, "tt_png_plan: record %lld is not a stripe's (end-of-block count %u, %llu tokens)", (long long)i, counts[256], (unsigned long long)tokens);
    int rc = tt_code_lengths("tt_png_plan", counts, TT_PNG_SYMS, TT_PNG_LIT_LIMIT, lengths);
    if (rc != TT_OK) return rc;
    int64_t bits = 0;
    rc = block_header("tt_png_plan", counts, lengths, headers + i * TT_PNG_HEADER_WORDS, TT_PNG_HEADER_WORDS, &bits);
    if (rc != TT_OK) return rc;
    reversed_codes(lengths, TT_PNG_SYMS, table);
    for (int s = 0; s < TT_PNG_SYMS; ++s) table[s] |= (uint32_t)lengths[s] << 16;
    table[286] = (uint32_t)((uint64_t)offset & 0xffffffffu);
    table[287] = (uint32_t)((uint64_t)offset >> 32);
    offset += (bits + 7) / 8 + 4;
  }
  *total_bytes_out = offset;
  return TT_OK;
}
